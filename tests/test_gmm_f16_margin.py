"""What storing GMM records as f16 costs a frame (CPU, oracle only).

An f16 GMM volume renders bit-identically to the oracle fed the same records
widened to float32 (tests/test_gpu_gmm_f16.py); what changes a frame is the
rounding of the records themselves.  This pins the documented bound (DESIGN.md
section 14): on the synthetic 24 x 20 x 16 volume (seed = K) at 96 x 72, density
0.05, cameras C0 and C1, the frame of the rounded records stays within two
RGBA8 steps, 2/255 per channel, of the float32 frame.  One step is too tight
for the variance (largest values measured over all (K, camera): method 1
0.00253, method 2 0.00551 > 1/255).  At density 0.6 early termination flips a
few rays' last sample and a frame moves by up to 0.018: that is not a bound
and is not asserted."""
import numpy as np
import pytest

CAMS = {"C0": None, "C1": (30.0, 45.0)}


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("K", [8, 16, 32])
@pytest.mark.parametrize("c", ["C0", "C1"])
def test_gmm_f16_rounding_stays_within_two_rgba8_steps(pkg, orc, c, K, method):
    dims = (24, 20, 16)
    wm, sg = orc.synth_gmm(*dims, K, seed=K)
    wwm = wm.astype(np.float16).astype(np.float32)
    wsg = sg.astype(np.float16).astype(np.float32)
    assert not np.array_equal(wm, wwm), "the rounding must change the records"
    assert not np.array_equal(sg, wsg), "the rounding must change the records"
    W, H = 96, 72
    m = pkg.camera.single_test_inv_view() if CAMS[c] is None else \
        pkg.camera.display_inv_view(CAMS[c])
    p = orc.make_params(W, H, m, query_method=method, density=0.05)
    a = orc.render_gmm(wm, sg, dims, p)["out_f"]
    b = orc.render_gmm(wwm, wsg, dims, p)["out_f"]
    err = float(np.max(np.abs(a - b)))
    print(f"K {K} {c} m{method}: max |dRGBA| = {err:.6f}")
    assert err <= 2.0 / 255.0, f"K {K} {c} m{method}: max |dRGBA| = {err}"
