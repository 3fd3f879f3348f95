"""Whole-frame numpy reference of the quantile query (method 11, DESIGN.md
section 17).  Test infrastructure.

The statistic is the inverse CDF of a record, bin i covering [i / B, (i + 1) / B)
with its mass spread uniformly, all in float32 and in this order:

    c_-1 = 0;  c_i = c_{i-1} + p_i  for i = 0 .. B-1
    T    = c_{B-1}
    tau  = q * T
    k    = the smallest i with c_i >= tau and p_i > 0; B-1 if there is none
    frac = p_k > 0 ? (tau - c_{k-1}) / p_k : 0
    frac = frac > 0 ? (frac > 1 ? 1 : frac) : 0
    Q    = (k + frac) * (1 / B)
    Q    = T > 0 ? Q : 0

which numpy float32 evaluates exactly as the kernel does (IEEE single precision,
correctly rounded division, no contraction, subnormals kept).  The spread is
Q(q_hi) - Q(q_lo), one float32 subtraction.  The frame is ref_numpy.render's
method-1 frame with its per-corner statistic, the module-level ref_numpy.stat,
replaced by that statistic for the duration of the call.
"""
import contextlib

import numpy as np

import ref_numpy

f32 = np.float32


def prefix_sums(p):
    """[c_0, .., c_{B-1}] of p (..., B) float32, each (...)"""
    p = np.asarray(p, dtype=np.float32)
    c, acc = [], np.zeros(p.shape[:-1], dtype=np.float32)
    for i in range(p.shape[-1]):
        acc = acc + p[..., i]
        c.append(acc)
    return c


def _quantile_of(p, c, q):
    nb = p.shape[-1]
    assert nb & (nb - 1) == 0, "1 / B must be exact"
    zero = np.zeros(p.shape[:-1], dtype=np.float32)
    T = c[nb - 1]
    tau = f32(q) * T
    k = np.full(p.shape[:-1], nb - 1, dtype=np.int64)
    found = np.zeros(p.shape[:-1], dtype=bool)
    for i in range(nb):
        here = ~found & (c[i] >= tau) & (p[..., i] > 0)
        k = np.where(here, i, k)
        found |= here
    cs = np.stack([zero] + c[:-1], axis=-1)  # c_{i-1}
    cp = np.take_along_axis(cs, k[..., None], axis=-1)[..., 0]
    pk = np.take_along_axis(p, k[..., None], axis=-1)[..., 0]
    num = tau - cp
    frac = np.where(pk > 0, num / np.where(pk > 0, pk, f32(1)), f32(0)).astype(np.float32)
    frac = np.where(frac > 0, np.where(frac > 1, f32(1), frac), f32(0)).astype(np.float32)
    Q = (k.astype(np.float32) + frac) * f32(1.0 / nb)
    return np.where(T > 0, Q, f32(0)).astype(np.float32)


def quantile_stat(p, q):
    """p: (..., B) float32 records; q: a float -> Q(q), or (lo, hi) -> Q(hi) - Q(lo);
    float32 (...)"""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(all="ignore"):
        c = prefix_sums(p)
        if np.ndim(q) == 0:
            return _quantile_of(p, c, q)
        lo, hi = q
        return (_quantile_of(p, c, hi) - _quantile_of(p, c, lo)).astype(np.float32)


@contextlib.contextmanager
def quantile_as_stat(q):
    """ref_numpy.stat = the quantile statistic inside the block, restored after it"""
    saved = ref_numpy.stat
    ref_numpy.stat = lambda p, comp: quantile_stat(p, q)
    try:
        yield
    finally:
        ref_numpy.stat = saved


def render(vol, q, W, H, m, **kw):
    """(packed RGBA8 (H, W) uint32, float RGBA (H, W, 4), samples per pixel (H, W),
    -1 = miss) of a method-11 frame of vol (nz, ny, nx, B): q a float for Q(q),
    (lo, hi) for the spread.  A float16 vol is widened (exactly) first, as the f16
    march widens it."""
    vol = np.asarray(vol).astype(np.float32)
    with quantile_as_stat(q):
        rgba, n = ref_numpy.render(vol, W, H, m, method=1, **kw)
    return ref_numpy.pack(rgba), rgba, n.astype(np.int32)
