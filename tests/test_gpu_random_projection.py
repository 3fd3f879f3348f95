"""Seeded random parity sweep of the projection march (k_march_proj, vr_project.hip,
DESIGN.md section 24): what test_gpu_random_transfer.py does for the table marches.

Every case is test_projection.proj_case's dict of its index: one of random_cases'
1-D table cases -- a record (fp32 or f16), codec or GMM volume whose nx may sit around
the planes' 15-voxel brick pitch with two, three or five rows, a camera that may sit
inside the volume or look along an axis, a frame of any size, a window that may be
negated, a table of any size whose entries may lie outside [0, 1], VR_TF_WIDE or an
occupancy cap -- with the mode dealt in turn; 40 whole frames, each rendered three
times (the estimate tile order, the order re-dealt by the recorded costs, the steady
one), and 8 multi-rank tile-list frames assembled by k_unscatter.  Every comparison
is exact: packed RGBA8, float RGBA and samples per pixel are np.array_equal to
tests/ref_projection.py marching the plane numpy computes per voxel (a GMM volume's
mean and variance planes excepted, as in test_gpu_random_transfer.py: the device's
own plane is marched).  tests/test_projection.py holds the census of the 48 reference
frames on the CPU.  A failure message carries the index and the whole case.
"""
import time

import numpy as np
import pytest

from test_gpu_random_queries import assert_same, render_frame, report, set_knobs
from test_gpu_random_transfer import bake_planes, frame_call
from test_projection import N_TILES, N_WHOLE, proj_case, proj_reference
from test_random_cases import camera
import random_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    """no projection, no table, no query state, no planes, no tuning knob, the default
    stream and no volume of any kind, before and after"""
    def drop():
        pkg.set_projection(None)
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
    return f"k_march_proj_{case['mode']}<B=1,M={13 if case['u'] == 13 else 0}>"


@pytest.mark.parametrize("index", range(N_WHOLE))
def test_random_projection_case(pkg, orc, gpu, tune, index):
    """a whole frame under a projection, three times"""
    import torch
    t0 = time.perf_counter()
    case = proj_case(index)
    what = f"case {index}: {case}"
    m = camera(pkg, case)
    planes = bake_planes(pkg, orc, case, what)
    pkg.set_transfer_function(rc.make_table(case["table"]))
    pkg.set_projection(case["mode"])
    set_knobs(tune, case)
    ref = proj_reference(case, planes, m)
    call, kw = frame_call(pkg, case)
    resident = pkg.layout_info()["resident_bytes"]
    for order in ("estimate order", "re-dealt order", "steady order"):
        got = render_frame(pkg, torch, dict(case, method=case["u"]), m, call, **kw)
        assert pkg.last_kernel() == kernel_name(case), f"{what}: {order}: {pkg.last_kernel()}"
        assert_same(got, ref, f"{what}, {order}")
    assert pkg.layout_info()["resident_bytes"] == resident, what  # no layout copy made
    report(dict(case, sweep="proj", seed=index), kernel_name(case), t0)


@pytest.mark.parametrize("index", range(N_WHOLE, N_WHOLE + N_TILES))
def test_random_projection_tile_list_case(pkg, orc, gpu, tune, index):
    """a multi-GPU split of a frame under a projection: every rank's tile list rendered
    into sentinel-filled packed slots, the slots assembled by k_unscatter"""
    import torch
    t0 = time.perf_counter()
    case = proj_case(index)
    what = f"case {index}: {case}"
    W, H, world = case["W"], case["H"], case["world"]
    m = camera(pkg, case)
    planes = bake_planes(pkg, orc, case, what)
    pkg.set_transfer_function(rc.make_table(case["table"]))
    pkg.set_projection(case["mode"])
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
    ref = proj_reference(case, planes, m)[0]
    assert np.array_equal(got, ref), f"{what}: {int(np.sum(got != ref))} pixels differ"
    report(dict(case, sweep="proj", seed=index), kernel_name(case), t0)
