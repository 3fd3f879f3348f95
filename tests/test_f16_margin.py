"""What storing the records as f16 costs a frame (CPU, oracle only).

An f16 volume renders bit-identically to the oracle fed the same records widened
to float32 (tests/test_gpu_f16.py); what changes a frame is the rounding of the
records themselves.  This pins the documented bound: on
the synthetic 24 x 20 x 16 volume at 96 x 72, camera C0, the frame of the rounded
records stays within one RGBA8 step, 1/255 per channel, of the float32 frame
(largest value measured: 0.0028)."""
import numpy as np
import pytest


@pytest.mark.parametrize("method", [1, 2, 3])
@pytest.mark.parametrize("nb", [4, 8, 32])
def test_f16_rounding_stays_within_one_rgba8_step(pkg, orc, nb, method):
    vol = orc.synth_volume(24, 20, 16, nb)
    widened = vol.astype(np.float16).astype(np.float32)
    assert not np.array_equal(vol, widened), "the rounding must change the records"
    W, H = 96, 72
    p = orc.make_params(W, H, pkg.camera.single_test_inv_view(), query_method=method)
    a = orc.render(vol, p)[1]
    b = orc.render(widened, p)[1]
    err = float(np.max(np.abs(a - b)))
    print(f"nb {nb} m{method}: max |dRGBA| = {err:.6f}")
    assert err <= 1.0 / 255.0, f"nb {nb} m{method}: max |dRGBA| = {err}"
