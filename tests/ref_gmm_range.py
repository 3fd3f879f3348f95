"""Numpy reference of the range probability of GMM volumes (query method 10 on a
GMM volume).  Test infrastructure.

The statistic of one voxel is restated from section 18.1 as a forward, vectorised
float32 evaluation over whole arrays of records: every multiply, add and the one
division are separate IEEE single-precision operations, which numpy float32
evaluates exactly as the kernels do (no contraction, subnormals kept).  The only
thing shared with the kernels' lane structure is the order of the sums: four
components in order, then the pairwise tree over the K / 4 partials.  The table
of E = Phi - 1/2 is the library's own, read through gmm_phi_table().

A frame is ref_numpy.render's method-1 frame of a (Z, Y, X, 1) volume that holds
the per-voxel statistic, with ref_numpy.stat replaced by "take that float" for
the duration of the call (the pattern of ref_weighted.weighted_stat): the GMM
march blends the 8 corner statistics exactly as the histogram march does.
"""
import contextlib

import numpy as np

import ref_numpy

f32 = np.float32


def phi_e(z, table):
    """E(z) = Phi(z) - 1/2 of float32 z (any shape); table = pkg.gmm_phi_table()"""
    c, nseg, h, zmax = table
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(all="ignore"):
        a = np.fmin(np.abs(z), f32(zmax))          # a NaN z takes ZMAX
        i = (a * f32(1.0 / h)).astype(np.int32)    # truncation; 0 <= i <= nseg
        t = a - i.astype(np.float32) * f32(h)
        e = c[2][i] + t * c[3][i]
        e = c[1][i] + t * e
        e = c[0][i] + t * e
    assert e.dtype == np.float32
    return np.copysign(e, z)


def tree_sum(p):
    """p (..., L) float32, L in 2, 4, 8 -> the pairwise sum T(p) of DESIGN.md 11.1"""
    p = np.asarray(p, dtype=np.float32)
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def range_stat(wm, sg, lo, hi, table):
    """wm (..., K, 2) and sg (..., K) records (float16 is widened first, exactly)
    -> float32 (...): the mass of every mixture in [lo, hi)"""
    wm = np.asarray(wm).astype(np.float32)
    sd = np.asarray(sg).astype(np.float32)
    w, mu = wm[..., 0], wm[..., 1]
    K = sd.shape[-1]
    assert K in (8, 16, 32) and w.shape == sd.shape
    lo, hi = f32(lo), f32(hi)
    with np.errstate(all="ignore"):
        r = f32(1) / sd
        ok = (sd > 0) & np.isfinite(r)
        eh = np.where(ok, phi_e((hi - mu) * r, table), np.where(mu < hi, f32(0.5), f32(-0.5)))
        el = np.where(ok, phi_e((lo - mu) * r, table), np.where(mu < lo, f32(0.5), f32(-0.5)))
        t = w * (eh - el)
        t = t.reshape(t.shape[:-1] + (K // 4, 4))
        p = t[..., 0]
        for j in (1, 2, 3):
            p = p + t[..., j]
        out = tree_sum(p)
    assert out.dtype == np.float32
    return out


@contextlib.contextmanager
def plane_stat():
    """ref_numpy.stat = the record's only float inside the block, restored after it"""
    saved = ref_numpy.stat
    ref_numpy.stat = lambda p, comp: p[..., 0]
    try:
        yield
    finally:
        ref_numpy.stat = saved


def render_plane(plane, W, H, m, **kw):
    """The frame of a (Z, Y, X) float32 plane of per-voxel statistics, as the dict
    oracle.render_gmm returns: out (H, W) uint32, out_f (H, W, 4), out_n (H, W)
    int32 with -1 where the ray misses the volume."""
    vol = np.asarray(plane, dtype=np.float32)[..., None]
    with plane_stat():
        rgba, n = ref_numpy.render(vol, W, H, m, method=1, **kw)
    return {"out": ref_numpy.pack(rgba), "out_f": rgba, "out_n": n.astype(np.int32)}


def render(wm, sg, lo, hi, table, W, H, m, **kw):
    """A whole method-10 frame of the GMM volume wm (Z, Y, X, K, 2), sg (Z, Y, X, K)"""
    return render_plane(range_stat(wm, sg, lo, hi, table), W, H, m, **kw)
