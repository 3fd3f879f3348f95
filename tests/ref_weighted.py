"""Whole-frame numpy reference of the weighted-bin query (method 10, DESIGN.md
section 16).  Test infrastructure.

The statistic is s = sum w_i p_i in float32 -- acc = 0, then acc = acc + p_i * w_i
for i = 0 .. B-1 in order, a separate multiply and add -- which numpy float32
evaluates exactly as the kernel does (IEEE single precision, no contraction,
subnormals kept).  The frame is ref_numpy.render's method-1 frame with its
per-corner statistic, the module-level ref_numpy.stat, replaced by that loop for
the duration of the call.
"""
import contextlib

import numpy as np

import ref_numpy

f32 = np.float32


def lin_stat(p, w):
    """p: (..., B) float32 records, w: B weights -> float32 (...)"""
    p = np.asarray(p, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    assert p.shape[-1] == w.size
    with np.errstate(all="ignore"):
        acc = np.zeros(p.shape[:-1], dtype=np.float32)
        for i in range(w.size):
            acc = acc + p[..., i] * w[i]
    return acc


def seeded_weights(n, seed=20261019):
    """n finite weights of both signs, uniform in [-1, 2), from a fixed seed"""
    rng = np.random.default_rng(seed + n)
    return rng.uniform(-1.0, 2.0, n).astype(np.float32)


@contextlib.contextmanager
def weighted_stat(w):
    """ref_numpy.stat = the weighted statistic inside the block, restored after it"""
    w = np.asarray(w, dtype=np.float32).reshape(-1).copy()
    saved = ref_numpy.stat
    ref_numpy.stat = lambda p, comp: lin_stat(p, w)
    try:
        yield
    finally:
        ref_numpy.stat = saved


def render(vol, w, W, H, m, **kw):
    """(packed RGBA8 (H, W) uint32, float RGBA (H, W, 4), samples per pixel (H, W),
    -1 = miss) of a method-10 frame of vol (nz, ny, nx, B) with weights w.  A
    float16 vol is widened (exactly) first, as the f16 march widens it."""
    vol = np.asarray(vol).astype(np.float32)
    with weighted_stat(w):
        rgba, n = ref_numpy.render(vol, W, H, m, method=1, **kw)
    return ref_numpy.pack(rgba), rgba, n.astype(np.int32)
