"""Whole-frame numpy reference of the level-crossing query (method 13, DESIGN.md
section 21).  Test infrastructure.

The sample of a cell is a joint function of its 8 corners,

    F_c = lin_stat(p_c, w)                        ref_weighted.lin_stat, per voxel
    lo  = F_0 * F_1 * ... * F_7                   left to right
    hi  = (1 - F_0) * (1 - F_1) * ... * (1 - F_7) left to right
    s   = (1 - lo) - hi

all in float32, one operation at a time, written over arrays (the corners are the
leading axis).  ref_numpy._render has the trilinear blend inline, so the march loop
is restated here (the ray set-up, the step, the transfer function and the
compositing of ref_numpy._render, methods 1/2/3) with the function that makes a
sample of the 8 corner values as an argument: `combine` for method 13, `trilinear`
for the frames of ref_weighted (tests/test_crossing.py holds the two loops against
each other bit for bit).
"""
import numpy as np

import ref_numpy
from ref_numpy import _lin, pack, transfer
from ref_weighted import lin_stat

f32 = np.float32


def combine(F, ax=None):
    """F: (8, ...) float32 corner values in gather order (x = c & 1, y = c & 2,
    z = c & 4) -> s (...) float32.  The filter weights ax are not used."""
    F = np.asarray(F, dtype=np.float32)
    with np.errstate(all="ignore"):
        lo = F[0]
        hi = f32(1) - F[0]
        for c in range(1, 8):
            lo = lo * F[c]
            hi = hi * (f32(1) - F[c])
        return ((f32(1) - lo) - hi).astype(np.float32)


def trilinear(F, ax):
    """the blend of ref_numpy._render: ax = the three _lin results"""
    lerp = ref_numpy._lerp
    c00 = lerp(F[0], F[1], ax[0][2])
    c10 = lerp(F[2], F[3], ax[0][2])
    c01 = lerp(F[4], F[5], ax[0][2])
    c11 = lerp(F[6], F[7], ax[0][2])
    return lerp(lerp(c00, c10, ax[1][2]), lerp(c01, c11, ax[1][2]), ax[2][2])


def render_plane(F, W, H, m, blend=combine, density=0.05, brightness=1.0, toff=0.0, tscale=1.0,
                 info=None):
    """(packed RGBA8 (H, W) uint32, float RGBA (H, W, 4), samples per pixel (H, W),
    -1 = miss) of a frame marched over the plane F (nz, ny, nx) of one float per
    voxel, each sample blend(the 8 corner values, the footprint).
    info: optional dict, receives early (H, W) bool (rays ended by opacity),
    samples and clamped (counts of samples taken / taken in a cell whose footprint
    the volume's edge clamps)."""
    with np.errstate(all="ignore"):
        return _march(np.asarray(F, dtype=np.float32), W, H, m, blend, density, brightness, toff,
                      tscale, info)


def _march(F, W, H, m, blend, density, brightness, toff, tscale, info):
    nz, ny, nx = F.shape
    M = np.asarray(m, dtype=np.float32).reshape(12)
    ys, xs = np.mgrid[0:H, 0:W]
    u = (xs.astype(np.float32) / f32(W)) * f32(2) - f32(1)
    v = (ys.astype(np.float32) / f32(H)) * f32(2) - f32(1)
    o = np.array([f32(0) * M[4 * r] + f32(0) * M[4 * r + 1] + f32(0) * M[4 * r + 2]
                  + f32(1) * M[4 * r + 3] for r in range(3)], dtype=np.float32)
    inv = f32(1) / np.sqrt(u * u + v * v + f32(-2) * f32(-2))
    d0 = [u * inv, v * inv, f32(-2) * inv]
    d = [d0[0] * M[4 * r] + d0[1] * M[4 * r + 1] + d0[2] * M[4 * r + 2] for r in range(3)]
    invR = [f32(1) / d[k] for k in range(3)]
    tb = [invR[k] * (f32(-1) - o[k]) for k in range(3)]
    tt = [invR[k] * (f32(1) - o[k]) for k in range(3)]
    tmn = [np.fmin(tt[k], tb[k]) for k in range(3)]
    tmx = [np.fmax(tt[k], tb[k]) for k in range(3)]
    tnear = np.fmax(np.fmax(tmn[0], tmn[1]), np.fmax(tmn[0], tmn[2]))
    tfar = np.fmin(np.fmin(tmx[0], tmx[1]), np.fmin(tmx[0], tmx[2]))
    hit = tfar > tnear
    tnear = np.where(tnear < 0, f32(0), tnear).astype(np.float32)
    pos = [o[k] + d[k] * tnear for k in range(3)]
    step = [d[k] * f32(0.01) for k in range(3)]
    t = tnear.copy()
    s = np.zeros((H, W, 4), dtype=np.float32)
    n = np.where(hit, 0, -1)
    active = hit.copy()
    early = np.zeros((H, W), dtype=bool)
    samples = clamped = 0
    dims = (nx, ny, nz)
    for i in range(500):
        if not active.any():
            break
        ax = [_lin(pos[k] * f32(0.5) + f32(0.5), dims[k]) for k in range(3)]
        vals = []
        for j in range(8):
            xi = ax[0][1] if j & 1 else ax[0][0]
            yi = ax[1][1] if j & 2 else ax[1][0]
            zi = ax[2][1] if j & 4 else ax[2][0]
            vals.append(F[zi, yi, xi])
        sample = blend(np.stack(vals), ax)
        edge = (ax[0][0] == ax[0][1]) | (ax[1][0] == ax[1][1]) | (ax[2][0] == ax[2][1])
        samples += int(active.sum())
        clamped += int((active & edge).sum())
        col = transfer((sample - f32(toff)) * f32(tscale))
        cw = col[..., 3] * f32(density)
        col = np.stack([col[..., 0] * cw, col[..., 1] * cw, col[..., 2] * cw, cw], -1)
        om = f32(1) - s[..., 3]
        ns = s + col * om[..., None]
        s = np.where(active[..., None], ns, s)
        n = np.where(active, i + 1, n)
        done = s[..., 3] > f32(0.95)
        early |= active & done
        t = np.where(active & ~done, t + f32(0.01), t).astype(np.float32)
        done |= t > tfar
        active &= ~done
        pos = [np.where(active, pos[k] + step[k], pos[k]).astype(np.float32) for k in range(3)]
    out = s * f32(brightness)
    out = np.where(out > 0, np.where(out > 1, f32(1), out), f32(0))
    out = np.where(hit[..., None], out, f32(0)).astype(np.float32)
    if info is not None:
        info.update(early=early, samples=samples, clamped=clamped)
    return pack(out), out, n.astype(np.int32)


def cdf_plane(vol, w):
    """F (nz, ny, nx) float32 of the records vol (nz, ny, nx, B) under the crossing
    weights w.  A float16 vol is widened (exactly) first, as the f16 march widens it."""
    return lin_stat(np.asarray(vol).astype(np.float32), w)


def render(vol, w, W, H, m, **kw):
    """a method-13 frame of vol (nz, ny, nx, B) with crossing weights w:
    render_plane's triple"""
    return render_plane(cdf_plane(vol, w), W, H, m, **kw)
