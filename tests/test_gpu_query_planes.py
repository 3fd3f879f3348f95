"""GPU checks of the life cycle the four record queries share (methods 10-13:
the weighted-bin, quantile, distance and level-crossing queries; DESIGN.md
sections 16, 17, 20, 21; 16.6 describes what they share on the host).

Each query has host state, a per-step march and an optional baked plane of one
float per voxel; the host library describes the four in one table and checks,
bakes, releases and launches them through one function each.  This module runs
the same sequence on every query: a refused bake leaves no plane, a bake is done
once, the plane has the size of a basicDataProcessing plane, and frames from the
plane, per step before it and per step after its release are the same frame --
the numpy reference's (tests/ref_*.py), bit for bit.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import ref_quantile
import ref_weighted
import test_crossing
import test_distance
from test_crossing import DIMS, H, THETA, W, camera, volume

pytestmark = pytest.mark.gpu

NB = 8
DTYPES = ("f32", "f16")
PIPE_PLANE = "k_march_pipe<B=1,M=0>"  # the plan's plane march of a row-aligned view


@functools.lru_cache(maxsize=None)
def _weighted_frame(dtype):
    return ref_weighted.render(volume(DIMS, NB, dtype), ref_weighted.seeded_weights(NB), W, H,
                               camera("C0"))


@functools.lru_cache(maxsize=None)
def _quantile_frame(dtype):
    return ref_quantile.render(volume(DIMS, NB, dtype), 0.5, W, H, camera("C0"))


def queries(pkg):
    """per query: the method, its calls, state of the volume's bin count and of
    another (None: the state has no bin count), the kernels of a C0 frame per step
    and from the plane, and the reference frame of a dtype"""
    return {
        "weighted": SimpleNamespace(
            method=pkg.QUERY_WEIGHTED, bake=pkg.bake_weighted, release=pkg.release_weighted,
            info=pkg.weighted_info, clear=lambda: pkg.set_bin_weights(None),
            set=lambda dtype: pkg.set_bin_weights(ref_weighted.seeded_weights(NB)),
            set_wrong=lambda: pkg.set_bin_weights(np.ones(4, np.float32)),
            step=f"k_march_lin<B={NB},M=10>", plane=PIPE_PLANE, frame=_weighted_frame),
        "quantile": SimpleNamespace(
            method=pkg.QUERY_QUANTILE, bake=pkg.bake_quantile, release=pkg.release_quantile,
            info=pkg.quantile_info, clear=lambda: pkg.set_quantile(None),
            set=lambda dtype: pkg.set_quantile(0.5), set_wrong=None,
            step=f"k_march_quant<B={NB},M=11>", plane=PIPE_PLANE, frame=_quantile_frame),
        "distance": SimpleNamespace(
            method=pkg.QUERY_DISTANCE, bake=pkg.bake_distance, release=pkg.release_distance,
            info=pkg.distance_info, clear=lambda: pkg.set_query_target(None),
            # (the reference's target is the centre record of the volume as resident)
            set=lambda dtype: pkg.set_query_target(test_distance.target(DIMS, NB, dtype), "emd"),
            set_wrong=lambda: pkg.set_query_target(
                test_distance.target(test_distance.SMALL, 4, "f32"), "emd"),
            step=f"k_march_dist<B={NB},M=12>", plane=PIPE_PLANE,
            frame=lambda dtype: test_distance.reference(DIMS, NB, dtype, "emd", False, "C0", W, H)),
        "crossing": SimpleNamespace(
            method=pkg.QUERY_CROSSING, bake=pkg.bake_crossing, release=pkg.release_crossing,
            info=pkg.crossing_info, clear=lambda: pkg.set_crossing_weights(None),
            set=lambda dtype: pkg.set_isovalue(THETA, NB),
            set_wrong=lambda: pkg.set_crossing_weights(test_crossing.weights(4)),
            step=f"k_march_cross<B={NB},M=13>", plane="k_march_cross_plane<B=1,M=13>",
            frame=lambda dtype: test_crossing.reference(DIMS, NB, dtype, "C0", W, H)),
    }


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    def clear():
        for q in queries(pkg).values():
            q.clear()
    clear()
    yield
    clear()
    pkg.release_stats()
    pkg.clear_tuning()


def render(pkg, torch, q):
    """one whole C0 frame of query q of the resident volume"""
    out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(H * W * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((H * W,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, W, H, camera("C0"), query_method=q.method, d_output_f=out_f,
                             d_steps=steps, transfer_scale=test_distance.DIST_TSCALE))
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(H, W),
            out_f.cpu().numpy().reshape(H, W, 4), steps.cpu().numpy().reshape(H, W))


def assert_same(got, want, what):
    for name, g, r in zip(("RGBA8", "float RGBA", "samples per pixel"), got, want):
        assert g.shape == r.shape, f"{what}: {name} shape"
        assert np.array_equal(g, r), f"{what}: {int(np.sum(g != r))} {name} values differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("weighted", "quantile", "distance", "crossing"))
def test_plane_life_cycle(pkg, gpu, name, dtype):
    import torch
    lib = pkg._lib
    q = queries(pkg)[name]
    assert test_distance.DIST_TSCALE == 1.0  # every reference frame is at transfer scale 1
    pkg.init_distribution(volume(DIMS, NB, dtype))
    # a refused bake leaves no plane: no state, then state of another bin count
    for prepare in (q.clear, q.set_wrong):
        if prepare is None:
            continue
        prepare()
        with pytest.raises(pkg.VRError) as e:
            q.bake()
        assert e.value.status == lib.VR_ERR_STATE
        assert q.info() == (None, 0)
    # the right state: the per-step frame is the reference's
    q.set(dtype)
    want = q.frame(dtype)[:3]
    assert (want[2] > 0).any()
    step = render(pkg, torch, q)
    assert pkg.last_kernel() == q.step
    assert_same(step, want, f"{name} {dtype} per step")
    # one bake makes the plane, of the size of a basicDataProcessing plane (both
    # are plane_pitches of the same grid); a second changes nothing
    q.bake()
    ptr, n = q.info()
    pkg.bake_stats()
    assert ptr and n == pkg.stats_info()[0][1]
    q.bake()
    assert q.info() == (ptr, n)
    baked = render(pkg, torch, q)
    assert pkg.last_kernel() == q.plane
    assert_same(baked, step, f"{name} {dtype} from the plane")
    # released: per step again, the same frame
    q.release()
    assert q.info() == (None, 0)
    again = render(pkg, torch, q)
    assert pkg.last_kernel() == q.step
    assert_same(again, baked, f"{name} {dtype} after the release")
