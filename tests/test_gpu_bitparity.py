"""Bit identity of the core marches on decode-magnifying scenes (GPU).

Methods 1/2/3/7, 4/5/6 and the GMM mean / variance each decode a voxel's
statistic in one of about a dozen hand-written copies (record_stat and kin,
box_stat / decode_box, wq_decode, stat_h, entropy_col / entropy_stash,
m7_rec_mean / m7q_decode, cq_stat / codec_stat_of, the gmm_stat variants).
Each must give the oracle's stats3 / codec_stats3 / GMM statistic to the last
bit.  The 1e-4 bar of test_gpu_parity.assert_parity does not see a last bit,
and at transfer_scale 1 not even word equality does.

Here every kernel family renders the scenes of tests/magnify.py -- narrow
transfer windows stepped across the statistic's range, on which
tests/test_magnified_scenes.py proves that one corner's statistic off by one
ulp changes pixels -- through the C ABI, and magnify.assert_bit_parity compares
d_output_f word for word, the RGBA8 frame and the samples per pixel with the
canonical oracle frame.  No tolerance.

Where the existing test of a path asserts the kernel's name, the same prefix is
asserted here, so a knob that stops selecting its kernel fails; everywhere the
kernel's name is in the failure message.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import magnify as M  # noqa: E402
from test_gpu_parity import test_every_kernel_path as _every_path  # noqa: E402

pytestmark = pytest.mark.gpu

_refs = {}      # (scene name, window) -> the canonical oracle frame, for every family
_resident = {}  # what the library holds, so a test uploads a volume once


def reference(scene, i, toff):
    key = (scene.name, i)
    if key not in _refs:
        M.orc().set_reading()
        _refs[key] = M.oracle_frame(scene, toff)
    return _refs[key]


def upload(pkg, scene):
    """make the scene's volume resident (per-step decode: no baked planes)"""
    key = (scene.kind, scene.size, scene.f16)
    if _resident.get("key") == key:
        return
    _resident["key"] = None
    vol = M.volume_f16(scene) if scene.f16 else M.volume(scene)
    if scene.kind == "hist":
        pkg.init_distribution(vol)
        assert pkg.volume_dtype() == ("f16" if scene.f16 else "f32")
    elif scene.kind == "codec":
        pkg.init_codec(*vol)
    else:
        pkg.init_gmm(*vol)
        assert pkg.gmm_dtype() == ("f16" if scene.f16 else "f32")
    _resident["key"] = key


@pytest.fixture(autouse=True)
def _fresh(pkg, gpu):
    """every test uploads its own volume and leaves no baked planes behind"""
    _resident["key"] = None
    yield
    _resident["key"] = None
    pkg.release_stats()


def render(pkg, torch, scene, toff):
    W, H = scene.W, scene.H
    out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(H * W * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((H * W,), -2, dtype=torch.int32, device="cuda")
    if scene.method == 7:
        size = scene.grid
    elif scene.kind == "hist":
        size = pkg.volume_info()[0]
    else:
        size = (1, 1, 1)
    d = pkg.make_desc(out, W, H, M.camera(scene.cam), density=scene.density,
                      transfer_offset=float(toff), transfer_scale=scene.tscale,
                      query_method=scene.method, volume_size=size, d_output_f=out_f,
                      d_steps=steps)
    if scene.kind == "gmm":
        pkg.render_gmm(d)
    else:
        pkg.render(d)
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(H, W),
            out_f.cpu().numpy().reshape(H, W, 4), steps.cpu().numpy().reshape(H, W))


def extra_windows(scene):
    """a scene whose proof needs fewer than 4 windows is also rendered through 4
    across the same range: more of the statistic's values under the same bar
    (outside the pinned counts)"""
    if scene.nwin >= 4:
        return []
    return list(M.windows(*M.stat_range(scene), 4, scene.tscale))


def hold(pkg, torch, scenes, what, want=None, load=True):
    """render every window of every scene and hold it to the oracle; want(scene) ->
    the regular expressions the kernel's name must match (a prefix as "^name<")"""
    assert scenes, what
    for scene in scenes:
        if load:
            upload(pkg, scene)
        for i, toff in enumerate(list(M.scene_windows(scene)) + extra_windows(scene)):
            got = render(pkg, torch, scene, toff)
            kern = pkg.last_kernel()
            for pattern in (want(scene) if want else ()):
                assert re.search(pattern, kern), f"{what} {scene.name}: {kern}, not {pattern}"
            if i == 0:
                print(f"{what} {scene.name}: {kern}")
            M.assert_bit_parity(got, reference(scene, i, toff),
                                f"{what} {scene.name} window {i} ({kern})")


def wide_kernels(s, mean_var=None):
    """what test_wide_records_take_batched_march asserts of 16 / 32 bins: mean and
    variance on k_march_wide (16 bins, row-aligned) or k_march_wq unless VR_WIDE
    says which; entropy on the quad march, oblique entropy of a volume coarse for
    the frame on the LDS box"""
    if s.method == 3:
        return ["^k_march<" if s.cam == "OBL" else "^k_march_wq<"]
    return [mean_var or ("^k_march_wide<" if (s.size, s.cam) == (16, "C0") else "^k_march_wq<")]


# the (VR_PATH, knobs) pairs of test_every_kernel_path, from its own parametrisation
PATHS = [m.args[1] for m in _every_path.pytestmark if m.args[0] == "path,env"][0]


@pytest.mark.parametrize("path,env", PATHS)
@pytest.mark.parametrize("nb", [4, 8])
def test_kernel_paths(pkg, gpu, path, env, nb, tune):
    """one-lane, quad, VR_QUAD2, LDS box (VR_BOX_MAX 0 / 64), VR_DUO 2/3/4, pipelined,
    VR_SEG +-2 / +-4 with and without VR_SEG_MAP, the VR_WG_PER_CU caps"""
    import torch
    tune.set("VR_PATH", path)
    for k, v in env.items():
        tune.set(k, v)
    hold(pkg, torch, M.select("hist", [nb], [1, 2, 3]), f"path {path} {env}")


@pytest.mark.parametrize("nb", [1, 2, 3, 4, 5, 8, 16, 32])
def test_default_dispatch(pkg, gpu, nb):
    """every bin count through the default dispatch: the compiled specialisations, the
    runtime-B path (3, 5), the wide records, the small-frame entropy dispatch"""
    import torch
    # (2- and 4-bin entropy of a small frame: the one-lane pipelined march, as
    # test_small_frame_entropy_dispatch asserts)
    def want(s):
        if nb in (16, 32):
            return wide_kernels(s)
        return ["^k_march_pipe<"] if s.method == 3 and nb in (2, 4) else []
    hold(pkg, torch, M.select("hist", [nb], [1, 2, 3]), f"default nb={nb}", want)


@pytest.mark.parametrize("wide", ["1", "2"])
@pytest.mark.parametrize("nb", [16, 32])
def test_wide_records(pkg, gpu, nb, wide, tune):
    """VR_WIDE=1: the lane-per-record k_march_wide; 2: the quad-cooperative k_march_wq
    (test_wide_records_take_batched_march); methods 1/2 take them, entropy keeps the
    default dispatch's kernels"""
    import torch
    tune.set("VR_WIDE", wide)
    name = "k_march_wide<" if wide == "1" else "k_march_wq<"
    hold(pkg, torch, M.select("hist", [nb], [1, 2, 3]), f"VR_WIDE={wide}",
         lambda s: wide_kernels(s, "^" + name))


@pytest.mark.parametrize("nb", [16, 32])
def test_wide_box_march(pkg, gpu, nb, tune):
    """16 / 32 bins on the LDS-box march: forced (VR_PATH=1), and through the dispatch
    as test_wide_coarse_rows_take_box_march reaches it (VR_SEG_RAYS=1000 puts these
    frames above the segmented threshold, and they hold >= 4 pixels per voxel of
    the face): row-aligned frames and entropy take k_march, the oblique mean and
    variance keep the quad-cooperative march"""
    import torch
    scenes = M.select("hist", [nb], [1, 2, 3])
    for s in scenes:
        assert s.W * s.H >= 4 * M.DIMS[0] * M.DIMS[1], "the frame must be coarse for the box"
    tune.set("VR_PATH", "1")
    hold(pkg, torch, scenes, "VR_PATH=1", lambda s: ["^k_march<"])
    tune.clear("VR_PATH")
    tune.set("VR_SEG_RAYS", "1000")
    hold(pkg, torch, scenes, "VR_SEG_RAYS=1000",
         lambda s: ["^k_march<" if s.cam == "C0" or s.method == 3 else "^k_march_wq<"])


@pytest.mark.parametrize("nb", [1, 8, 32])
def test_f16_records(pkg, gpu, nb):
    """k_march_pipe_h against the oracle on the widened records"""
    import torch
    hold(pkg, torch, M.select("hist", [nb], f16=True), "f16", lambda s: ["^k_march_pipe_h<"])


@pytest.mark.parametrize("path,env", [("", {}), ("2", {}), ("7", {"VR_SEG": "-2"}),
                                      ("7", {"VR_SEG": "4"}), ("1", {}),
                                      ("", {"VR_PLANE8": "0"})])
def test_baked_planes(pkg, gpu, path, env, tune):
    """bake_stats(), then the frames filter the planes: VR_PATH 2 / 7 / 1 (1 is ignored
    for the bricked planes), the oblique views' 8 x 2 x 2 plane copy and without it;
    method 7 from the baked corner means"""
    import torch
    if path:
        tune.set("VR_PATH", path)
    for k, v in env.items():
        tune.set(k, v)
    scenes = M.select("hist", [8], [1, 2, 3, 7])
    upload(pkg, scenes[0])
    pkg.bake_stats()

    def want(s):
        pats = ["M=0|M=-"]
        if s.method == 7:
            if not path and not env:
                pats.append("B=1,M=-7>")
        elif s.cam != "C0" and path in ("", "2"):
            pats.append("plane8" if not env else "^(?!.*plane8)")
        return pats
    hold(pkg, torch, scenes, f"baked path {path!r} {env}", want, load=False)


@pytest.mark.parametrize("quad", ["1", "0"])
def test_method7(pkg, gpu, quad, tune):
    """method 7's quad-cooperative and one-lane pipelined marches on oblique views
    (test_method7_oblique_kernels' knob), the row-aligned view, a grid that is not
    the volume's"""
    import torch
    tune.set("VR_M7_QUAD", quad)
    name = "k_march_m7_quad" if quad == "1" else "k_march_m7_pipe"
    hold(pkg, torch, M.select("hist", [8], [7]), f"VR_M7_QUAD={quad}",
         lambda s: ["^" + name] if s.cam != "C0" and s.grid == M.DIMS else [])


@pytest.mark.parametrize("cmap", ["", "1"])
@pytest.mark.parametrize("nb", [8, 32])
def test_codec(pkg, gpu, nb, cmap, tune):
    """methods 4/5/6: the default dispatch and the 16 x 4 pixel block map"""
    import torch
    if cmap:
        tune.set("VR_CODEC_MAP", cmap)
    hold(pkg, torch, M.select("codec", [nb]), f"codec map {cmap!r}",
         lambda s: [] if cmap else ["^k_march_codec"])


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_gmm(pkg, gpu, K, f16):
    """GMM mean and variance, whole volume, float32 and f16 records"""
    import torch
    name = "^k_march_gmm_h<" if f16 else "^k_march_gmm<"

    def want(s):
        return [name, f"<B={K},M={s.method}>"]
    try:
        hold(pkg, torch, M.select("gmm", [K], f16=f16), "gmm", want)
    finally:
        pkg.free_gmm()
