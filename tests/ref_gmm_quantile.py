"""Numpy reference of the quantile of GMM volumes (query method 11 on a GMM volume,
DESIGN.md section 19).  Test infrastructure.

The statistic of one voxel is restated from section 19.1 as a vectorised float32
evaluation over whole arrays of records: the reciprocals once, the bracket
[a0, b0] over the components of positive weight, and N bisections, each one
evaluation of the table CDF C(mid) over all records at once.  Every multiply, add
and division is a separate IEEE single-precision operation, which numpy float32
evaluates exactly as the kernels do.  Shared with the kernels' lane structure is
only the order of the sums: four components in order, then the pairwise tree over
the K / 4 partials (ref_gmm_range.tree_sum).  E = Phi - 1/2 is
ref_gmm_range.phi_e on the library's own table (gmm_phi_table()), and N is the
library's (gmm_quantile_steps()): neither is restated here.

A frame is ref_gmm_range.render_plane of the per-voxel statistic.
"""
import numpy as np

from ref_gmm_range import phi_e, render_plane, tree_sum

f32 = np.float32


def _seq4(t):
    """(..., K) terms -> (..., K / 4) lane partials, four in order"""
    t = t.reshape(t.shape[:-1] + (t.shape[-1] // 4, 4))
    p = t[..., 0]
    for j in (1, 2, 3):
        p = p + t[..., j]
    return p


class Mixtures:
    """The per-record values every search of the same records shares: r, the Dirac
    flags, W, the bracket and whether any weight is positive."""

    def __init__(self, wm, sg, table):
        wm = np.asarray(wm).astype(np.float32)      # float16 widens exactly
        self.sd = np.asarray(sg).astype(np.float32)
        self.w, self.mu = wm[..., 0], wm[..., 1]
        K = self.sd.shape[-1]
        assert K in (8, 16, 32) and self.w.shape == self.sd.shape
        self.table = table
        zmax = f32(table[3])
        with np.errstate(all="ignore"):
            self.r = f32(1) / self.sd
            self.ok = (self.sd > 0) & np.isfinite(self.r)
            pos = self.w > 0
            reach = zmax * self.sd
            self.a0 = np.fmin.reduce(np.where(pos, self.mu - reach, f32(np.inf)), axis=-1)
            self.b0 = np.fmax.reduce(np.where(pos, self.mu + reach, f32(-np.inf)), axis=-1)
            self.live = pos.any(-1)
            self.W = tree_sum(_seq4(self.w))
        assert self.a0.dtype == self.b0.dtype == self.W.dtype == np.float32

    def cdf(self, x):
        """C(x) of the table, x float32 of the records' shape"""
        x = np.asarray(x, np.float32)[..., None]
        with np.errstate(all="ignore"):
            e = np.where(self.ok, phi_e((x - self.mu) * self.r, self.table),
                         np.where(self.mu < x, f32(0.5), f32(-0.5)))
            c = self.w * (f32(0.5) + e)
            out = tree_sum(_seq4(c))
        assert out.dtype == np.float32
        return out

    def quantile(self, q, steps):
        with np.errstate(all="ignore"):
            tau = f32(q) * self.W
            lo, hi = self.a0.copy(), self.b0.copy()
            for _ in range(steps):
                mid = (lo + hi) * f32(0.5)
                below = self.cdf(mid) < tau
                lo = np.where(below, mid, lo)
                hi = np.where(below, hi, mid)
        out = np.where(self.live, hi, f32(0))
        assert out.dtype == np.float32
        return out


def quantile_stat(wm, sg, q_lo, q_hi, spread, table, steps):
    """wm (..., K, 2) and sg (..., K) records -> float32 (...): Q(q_lo), or
    Q(q_hi) - Q(q_lo) when spread (one float subtraction)"""
    mix = Mixtures(wm, sg, table)
    q = mix.quantile(q_lo, steps)
    if spread:
        with np.errstate(all="ignore"):
            q = mix.quantile(q_hi, steps) - q
    return q


def render(wm, sg, q_lo, q_hi, spread, table, steps, W, H, m, **kw):
    """A whole method-11 frame of the GMM volume wm (Z, Y, X, K, 2), sg (Z, Y, X, K)"""
    return render_plane(quantile_stat(wm, sg, q_lo, q_hi, spread, table, steps), W, H, m, **kw)
