"""Whole-frame numpy reference of the distribution-distance query (method 12,
DESIGN.md section 20).  Test infrastructure.

The statistic is the distance of a record p from a target record h, all in
float32.  It is stated here in arrays, not in the kernel's running scalars:

    d   = p - h                          the bin differences, (..., B)
    E   = the prefix sums of d           E_0 = 0 + d_0, E_i = E_{i-1} + d_i
    L1  = (sum of |d_i|) * 0.5
    EMD = (sum of |E_i|) * (1 / B)       B a power of two: an exact scale
    KS  = the fmax of the |E_i|          from 0; np.fmax: the other operand for a NaN
    s   = 1 - D for the similarity, else D

with every sum and the fmax taken in bin order from 0, one float32 operation at a
time, which numpy float32 evaluates exactly as the kernel does (IEEE single
precision, no contraction, subnormals kept).  The frame is ref_numpy.render's
method-1 frame with its per-corner statistic, the module-level ref_numpy.stat,
replaced by that statistic for the duration of the call.
"""
import contextlib

import numpy as np

import ref_numpy

f32 = np.float32
METRICS = ("l1", "emd", "ks")


def differences(p, h):
    """d (..., B) float32 = p - h"""
    p = np.asarray(p, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32).reshape(-1)
    assert p.shape[-1] == h.size, (p.shape, h.size)
    return (p - h).astype(np.float32)


def prefix(d):
    """E (..., B) float32: the running sums of d along the last axis, from 0"""
    E = np.empty_like(d)
    acc = np.zeros(d.shape[:-1], dtype=np.float32)
    for i in range(d.shape[-1]):
        acc = acc + d[..., i]
        E[..., i] = acc
    return E


def _ordered(a, op):
    """op folded over the last axis of a in order, from 0"""
    acc = np.zeros(a.shape[:-1], dtype=np.float32)
    for i in range(a.shape[-1]):
        acc = op(acc, a[..., i]).astype(np.float32)
    return acc


def distance_stat(p, h, metric="l1", similarity=False):
    """p: (..., B) float32 records, h: B floats -> float32 (...)"""
    assert metric in METRICS, metric
    with np.errstate(all="ignore"):
        d = differences(p, h)
        nb = d.shape[-1]
        assert nb & (nb - 1) == 0, "1 / B must be exact"
        if metric == "l1":
            D = _ordered(np.abs(d), np.add) * f32(0.5)
        elif metric == "emd":
            D = _ordered(np.abs(prefix(d)), np.add) * f32(1.0 / nb)
        else:
            D = _ordered(np.abs(prefix(d)), np.fmax)
        D = np.asarray(D, dtype=np.float32)
        return (f32(1.0) - D).astype(np.float32) if similarity else D


def region_mean(vol, lo, hi):
    """the mean record of the box [lo, hi) = [x0, x1) x [y0, y1) x [z0, z1) of vol
    (nz, ny, nx, B): each bin summed in float64, voxel after voxel, x fastest, then
    y, then z, divided by the voxel count in float64 and rounded once to float32.
    A float16 vol is widened (exactly) first."""
    vol = np.asarray(vol)
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    nb = vol.shape[-1]
    total = [0.0] * nb  # Python floats are IEEE doubles
    count = 0
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                for i in range(nb):
                    total[i] = total[i] + float(np.float32(vol[z, y, x, i]))
                count += 1
    assert count > 0
    return np.array([np.float32(t / float(count)) for t in total], dtype=np.float32)


@contextlib.contextmanager
def distance_as_stat(h, metric, similarity):
    """ref_numpy.stat = the distance statistic inside the block, restored after it"""
    saved = ref_numpy.stat
    ref_numpy.stat = lambda p, comp: distance_stat(p, h, metric, similarity)
    try:
        yield
    finally:
        ref_numpy.stat = saved


def render(vol, h, metric, similarity, W, H, m, **kw):
    """(packed RGBA8 (H, W) uint32, float RGBA (H, W, 4), samples per pixel (H, W),
    -1 = miss) of a method-12 frame of vol (nz, ny, nx, B) against the target h.  A
    float16 vol is widened (exactly) first, as the f16 march widens it."""
    vol = np.asarray(vol).astype(np.float32)
    with distance_as_stat(h, metric, similarity):
        rgba, n = ref_numpy.render(vol, W, H, m, method=1, **kw)
    return ref_numpy.pack(rgba), rgba, n.astype(np.int32)
