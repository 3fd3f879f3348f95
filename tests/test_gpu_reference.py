"""The HIP library against the reference's own kernels, built for the CPU.

The frame the library renders through the reference's entry points (initCuda,
copyInvViewMatrix, basicDataProcessing, render_kernel, freeCudaBuffers) is
compared, RGBA8 word for word, with the frame the reference's d_render computes on
the host in the same test (oracle/_ref/libref_*.so, built by oracle/ref/build_ref.py
from the reference's kernel text).  The same frame through the library's own
descriptor is compared on the float RGBA words too: the reference packs a
saturated float RGBA that it never stores, and the shim keeps it.  No oracle is
involved: this is the product against the reference, under the shim's reading
of the texture unit, rsqrtf and log(float) (oracle/ref/shim/helper_cuda.h).

The libraries are CPU code and are not committed; where they are not there (a
checkout on a machine that never saw the reference) the module skips.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as graft  # noqa: E402
import magnify  # noqa: E402

pytestmark = pytest.mark.gpu

R = graft.load_reference()
if not (R.available("b32") and R.available("b8")):
    pytest.skip("oracle/_ref/libref_b32.so / libref_b8.so not built (no reference directory "
                "where build() ran)", allow_module_level=True)

NX, NY, NZ = R.DIMS
W, H = 64, 48
PREFILL = 0x5AA5C33C  # a miss writes nothing (K:302-303)
DEFAULT = dict(density=0.05, brightness=1.0, transfer_offset=0.0, transfer_scale=1.0)


def spiky32():
    """every voxel its own spiky 32-bin histogram, a tenth of the bins exactly 0"""
    rng = np.random.default_rng(4032)
    p = rng.random((NZ, NY, NX, 32))
    p = p * p * p
    p[rng.random(p.shape) < 0.1] = 0.0
    p[..., 0] += 1e-3
    p /= magnify._total(p)
    return p


@pytest.fixture(scope="module")
def scenes(orc):
    """nb -> (records float32 (10, 50, 50, nb), codec arrays); the 8-bin records are
    the 32-bin ones with every four neighbouring bins summed"""
    p32 = spiky32()
    p8 = p32.reshape(NZ, NY, NX, 8, 4)
    p8 = p8[..., 0] + p8[..., 1] + p8[..., 2] + p8[..., 3]
    out = {}
    for nb, p in ((32, p32), (8, p8)):
        vol = np.ascontiguousarray(p.astype(np.float32))
        codec = orc.synth_codec(NX, NY, NZ, nb, seed=77 + nb)  # numpy only; bin ids in range
        for a in (vol,) + codec:
            a.setflags(write=False)
        out[nb] = (vol, codec)
    return out


def param_sets(values):
    """the default parameters and two narrow windows (transfer_scale 256, density
    0.5) inside the statistic's 10th-90th percentile"""
    lo, hi = magnify._p10_p90(np.asarray(values, np.float32))
    return [DEFAULT] + [dict(density=0.5, brightness=1.0, transfer_offset=float(t),
                             transfer_scale=256.0) for t in magnify.windows(lo, hi, 2, 256.0)]


@pytest.mark.parametrize("nb", [32, 8])
def test_library_renders_what_the_reference_text_computes(pkg, orc, gpu, scenes, nb):
    import torch
    vol, codec = scenes[nb]
    ref = R.load(f"b{nb}")
    ref.set_weight_trunc(False)
    ref.init(vol, codec)
    plane, cplane = ref.basic_data_processing()
    # method 7 samples 50 x the corner mean (K:479); the plane's .x is mean / 0.0217
    values = {1: plane[:, 0], 2: plane[:, 1], 3: plane[:, 2],
              7: plane[:, 0] * np.float32(0.0217 * 50.0),
              4: cplane[:, 0], 5: cplane[:, 1], 6: cplane[:, 2]}
    pkg.initCuda(vol.reshape(-1), R.DIMS, (nb, NX * NY, NZ))
    pkg.init_codec(*codec)
    pkg.basicDataProcessing()
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    out2 = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    steps = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    grid, block = ((W + 15) // 16, (H + 15) // 16, 1), (16, 16, 1)
    bad = []
    frames = 0
    try:
        for cname in ("C0", "OBL"):
            m = magnify.camera(cname)
            pkg.copyInvViewMatrix(m, 48)
            for method in (1, 2, 3, 7, 4, 5, 6):
                for kw in param_sets(values[method]):
                    out.fill_(PREFILL)  # (below 2^31: the same int32 word)
                    pkg.render_kernel(grid, block, out, W, H, kw["density"], kw["brightness"],
                                      kw["transfer_offset"], kw["transfer_scale"], method,
                                      R.DIMS)
                    torch.cuda.synchronize()
                    got = out.cpu().numpy().view(np.uint32).reshape(H, W)
                    p = orc.make_params(W, H, m, query_method=method, m7_dims=R.DIMS, **kw)
                    want, want_f = ref.render(p, prefill=PREFILL, want_float=True)
                    frames += 1
                    n = int(np.sum(got != want))
                    if n:
                        bad.append(f"{cname} method {method} {kw}: {n} pixels")
                    # the library's own descriptor: float RGBA words and which rays hit
                    out2.fill_(PREFILL)
                    out_f.zero_()
                    steps.fill_(-2)
                    pkg.render(pkg.make_desc(out2, W, H, m, query_method=method,
                                             volume_size=R.DIMS, d_output_f=out_f, d_steps=steps,
                                             **kw))
                    torch.cuda.synchronize()
                    gf = out_f.cpu().numpy().reshape(H, W, 4)
                    hit = steps.cpu().numpy().reshape(H, W) >= 0
                    written = ~np.isnan(want_f).any(axis=-1)
                    nf = int(np.sum(hit != written))
                    both = hit & written
                    nf += int(np.sum(np.any(gf[both].view(np.uint32) !=
                                            want_f[both].view(np.uint32), axis=-1)))
                    n2 = int(np.sum(out2.cpu().numpy().view(np.uint32).reshape(H, W) != want))
                    if nf or n2:
                        bad.append(f"{cname} method {method} {kw} through the descriptor: "
                                   f"{n2} RGBA8 pixels, {nf} float pixels")
                    assert np.any(want == PREFILL) and np.any(want != PREFILL)
    finally:
        pkg.freeCudaBuffers()
    print(f"{nb} bins: {frames} frames, {len(bad)} differ")
    assert not bad, f"{len(bad)} of {frames} frames differ from the reference's d_render: {bad[:4]}"
