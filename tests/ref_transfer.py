"""Whole-frame numpy reference of frames classified through a user-defined
transfer function.  Test infrastructure.

A table of n RGBA float32 entries is sampled as the built-in nine are
(ref_numpy.transfer): ref_numpy._lin with n for 9, then ref_numpy._lerp per
channel, nothing in the table clamped.  The march is ref_crossing._march, not
restated here: render_plane binds ref_crossing.transfer to the table's classifier
for the duration of the call.
"""
import numpy as np

import ref_crossing
from ref_numpy import _lerp, _lin

f32 = np.float32


def transfer_table(x, table):
    """x (...) -> RGBA (..., 4) float32 of the (n, 4) table at the normalised
    coordinate x (clamped to [0, 1], NaN as 0)"""
    t = np.asarray(table, dtype=np.float32)
    assert t.ndim == 2 and t.shape[1] == 4 and 1 <= t.shape[0] <= 256, t.shape
    with np.errstate(all="ignore"):
        i0, i1, a = _lin(np.asarray(x, dtype=np.float32), t.shape[0])
        return _lerp(t[i0], t[i1], a[..., None]).astype(np.float32)


def render_plane(F, W, H, m, table, blend=ref_crossing.combine, **kw):
    """ref_crossing.render_plane's triple (RGBA8, float RGBA, samples per pixel) of
    the plane F (nz, ny, nx) with every sample classified through `table`; blend:
    ref_crossing.combine (method 13) or ref_crossing.trilinear (every other plane).
    kw: density, brightness, toff, tscale, info, as there."""
    saved = ref_crossing.transfer
    ref_crossing.transfer = lambda x: transfer_table(x, table)
    try:
        return ref_crossing.render_plane(F, W, H, m, blend=blend, **kw)
    finally:
        ref_crossing.transfer = saved
