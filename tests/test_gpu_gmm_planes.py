"""GPU checks of the life cycle the three GMM plane sets share: the mean /
variance planes, the range plane and the quantile plane (DESIGN.md sections 15,
18, 19; 16.7 describes what they share on the device and on the host).

Each set has a per-step march, a bake of the resident slices into whole-volume
planes and frames from those planes; the host library describes the three in one
table and bakes, releases, reports and launches them through one function each,
and the bake kernels share one body.  This module runs the same sequence on every
set -- the counterpart of test_gpu_query_planes for the record queries: unset
state refuses, the per-step frame is the reference's, one bake makes the planes,
frames from them are the reference's, a partial bake refuses a frame, and after
the release the per-step frame is what it was.

The volume, the frame size, the references and the comparisons are those of
test_gpu_gmm_baked, test_gpu_gmm_range and test_gpu_gmm_quantile (bit identity):
37 x 11 x 9, where 37 is no multiple of the 32 / 16 / 8 voxels a wave bakes at
K = 8 / 16 / 32, so a row ends in clamped lanes and a partly empty last wave."""
from types import SimpleNamespace

import pytest

import ref_crossing
import test_gpu_gmm_baked as gb
import test_gpu_gmm_quantile as gq
import test_gpu_gmm_range as gr
from test_gpu_crossing import PLANE_KERNEL as CROSS_PLANE, assert_same
from test_gpu_gmm_f16 import Frame, cam, check, same
from test_gpu_gmm_range import DIMS, H, W

pytestmark = pytest.mark.gpu

RANGE = gr.RANGES[3]   # (-inf, 0.3): the plane is also the F = P(v < 0.3) method 13 reads
Q = 0.5
EMPTY = ((0, 0, 0), None, 0, 0)


def plane_sets(pkg, orc, K, dtype, c):
    """per set: its calls, the state it needs (None: none), the methods that march
    per step, the kernel of that march, the check of the baked planes, and the
    reference frame of a method at camera c"""
    h = "_h" if dtype == "f16" else ""
    return {
        "stats": SimpleNamespace(
            bake=pkg.bake_gmm_stats, release=pkg.release_gmm_stats, info=pkg.gmm_stats_info,
            set=None, clear=None, methods=(1, 2), step="k_march_gmm" + h,
            planes=lambda what: gb.assert_planes(pkg, gb.want_planes(orc, K, dtype), what),
            frame=lambda method: gb.want_frame(orc, pkg, K, dtype, c, method, 0.05)),
        "range": SimpleNamespace(
            bake=pkg.bake_gmm_range, release=pkg.release_gmm_range, info=pkg.gmm_range_info,
            set=lambda: pkg.set_gmm_range(*RANGE), clear=pkg.clear_gmm_range, methods=(10,),
            step="k_march_gmm_range" + h,
            planes=lambda what: gr.assert_plane(
                pkg, gr.want_plane(orc, pkg, DIMS, K, dtype, RANGE), DIMS, what),
            frame=lambda method: gr.want_frame(orc, pkg, DIMS, K, dtype, RANGE, c, 0.05)),
        "quantile": SimpleNamespace(
            bake=pkg.bake_gmm_quantile, release=pkg.release_gmm_quantile,
            info=pkg.gmm_quantile_info, set=lambda: pkg.set_quantile(Q),
            clear=lambda: pkg.set_quantile(None), methods=(11,), step="k_march_gmm_quant" + h,
            planes=lambda what: gq.assert_plane(
                pkg, gq.want_plane(orc, pkg, DIMS, K, dtype, Q), DIMS, what),
            frame=lambda method: gq.want_frame(orc, pkg, DIMS, K, dtype, Q, c, 0.05)),
    }


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    """no GMM planes, no range, no quantile and no GMM volume in either slot, before
    and after"""
    def drop():
        pkg.set_quantile(None)
        pkg.clear_gmm_range()
        pkg.release_gmm_stats()
        for slot in (1, 0):
            pkg.gmm_select(slot)
            pkg.free_gmm()
    drop()
    yield
    drop()


def frame(pkg, torch, call, m, method):
    f = Frame(pkg, torch, W, H, m, method)
    call(f.desc)
    torch.cuda.synchronize()
    return f.get()


def refused(pkg, call, *args):
    with pytest.raises(pkg.VRError) as e:
        call(*args)
    assert e.value.status == pkg._lib.VR_ERR_STATE


# K = 16 with both element types; K = 8 and K = 32 with one each
@pytest.mark.parametrize("K,dtype", [(16, "f32"), (16, "f16"), (8, "f16"), (32, "f32")])
@pytest.mark.parametrize("name", ("stats", "range", "quantile"))
def test_plane_set_life_cycle(pkg, orc, gpu, name, K, dtype):
    import torch
    c = "C0" if dtype == "f32" else "C1"   # a row-aligned and an oblique view
    m = cam(pkg, c)
    s = plane_sets(pkg, orc, K, dtype, c)[name]
    what = f"{name} K={K} {dtype} {c}"
    (wm, sg), _ = gr.records(orc, DIMS, K, dtype)
    pkg.init_gmm(wm, sg)
    assert pkg.gmm_dtype() == dtype
    # 1. without the set's state: no bake, no per-step frame, no plane
    if s.clear:
        s.clear()
        refused(pkg, s.bake)
        refused(pkg, pkg.render_gmm, Frame(pkg, torch, W, H, m, s.methods[0]).desc)
    assert s.info() == EMPTY
    # 2. with it: the per-step frames are the reference's
    if s.set:
        s.set()
    steps = {}
    for method in s.methods:
        steps[method] = frame(pkg, torch, pkg.render_gmm, m, method)
        assert pkg.last_kernel() == f"{s.step}<B={K},M={method}>"
        check(steps[method], s.frame(method), f"{what} m{method} per step")
    # 3. one bake makes the planes, of the size of the mean / variance planes (all
    # are plane_pitches of the same grid), every slice baked; a second keeps them
    s.bake()
    dims, ptr, n, nbaked = s.info()
    pkg.bake_gmm_stats()
    assert ptr and tuple(dims) == DIMS and nbaked == DIMS[2] and n == pkg.gmm_stats_info()[2]
    assert n == gb.plane_pitches(DIMS[0], DIMS[1])[1] * DIMS[2]
    s.planes(what)
    s.bake()
    assert s.info() == (dims, ptr, n, nbaked)
    # 4. frames from the planes: the reference's, by a plane march; method 13 reads
    # the range plane through the crossing combine
    for method in s.methods:
        got = frame(pkg, torch, pkg.render_gmm_baked, m, method)
        kernel = pkg.last_kernel()
        assert "<B=1,M=0>" in kernel and kernel.startswith(("k_march_pipe", "k_march_seg")), kernel
        check(got, s.frame(method), f"{what} m{method} from the planes")
        same(got, steps[method], f"{what} m{method}: planes against per step")
    if name == "range":
        got = frame(pkg, torch, pkg.render_gmm_baked, m, 13)
        assert pkg.last_kernel() == CROSS_PLANE
        F = gr.want_plane(orc, pkg, DIMS, K, dtype, RANGE)
        assert_same(got, ref_crossing.render_plane(F, W, H, m), f"{what} m13 from the plane")
    # 5. fresh planes baked from slices [0, 5) alone: five slices, no frame
    s.release()
    pkg.init_gmm(wm[:5], sg[:5], DIMS, z_base=0)
    s.bake()
    assert tuple(s.info()[0]) == DIMS and s.info()[3] == 5
    for method in s.methods:
        refused(pkg, pkg.render_gmm_baked, Frame(pkg, torch, W, H, m, method).desc)
    # 6. released: no planes, no frame from them, and per step the same frames
    s.release()
    assert s.info() == EMPTY
    pkg.init_gmm(wm, sg)
    for method in s.methods:
        refused(pkg, pkg.render_gmm_baked, Frame(pkg, torch, W, H, m, method).desc)
        same(frame(pkg, torch, pkg.render_gmm, m, method), steps[method],
             f"{what} m{method} per step after the release")
        assert pkg.last_kernel() == f"{s.step}<B={K},M={method}>"
