"""slabs.max_slices_for with f16 GMM records (CPU): a record of 6 bytes per
component instead of 12, so the same HBM holds what twice the HBM holds in
fp32 -- up to the halo slice, which is subtracted once either way."""
import inspect

import pytest


@pytest.mark.parametrize("nx,ny,K,hbm,reserve", [
    (2048, 2048, 16, 288e9, 0.1), (1024, 1024, 16, 288e9, 0.1), (512, 512, 32, 64e9, 0.25),
    (300, 200, 8, 1e9, 0.0), (24, 20, 16, 1e6, 0.1)])
def test_f16_slab_holds_what_twice_the_hbm_holds_in_fp32(pkg, nx, ny, K, hbm, reserve):
    S = pkg.slabs
    f16 = S.max_slices_for(nx, ny, K, hbm, reserve, dtype="f16")
    # slices + halo that fit: floor(hbm (1 - reserve) / (nx ny 6 K)) - 1
    assert f16 == int(hbm * (1 - reserve) // (nx * ny * 6 * K)) - 1
    # fp32 with twice the HBM: the same quotient (2 hbm / 12 K = hbm / 6 K), the
    # same one halo slice taken off
    assert f16 == S.max_slices_for(nx, ny, K, 2 * hbm, reserve)
    f32 = S.max_slices_for(nx, ny, K, hbm, reserve)
    # (f32 + 1) slices of 12 K bytes fit, so 2 (f32 + 1) of 6 K do; one more pair cannot
    assert 2 * (f32 + 1) - 1 <= f16 <= 2 * (f32 + 1)


def test_default_is_fp32_and_unchanged(pkg):
    S = pkg.slabs
    assert inspect.signature(S.max_slices_for).parameters["dtype"].default == "f32"
    for nx, ny, K, hbm in ((2048, 2048, 16, 288e9), (1024, 1024, 8, 100e9)):
        want = int(hbm * 0.9 // (nx * ny * 12 * K)) - 1
        assert S.max_slices_for(nx, ny, K, hbm) == want
        assert S.max_slices_for(nx, ny, K, hbm, dtype="f32") == want
    with pytest.raises(ValueError):
        S.max_slices_for(64, 64, 16, 1e9, dtype="bf16")
