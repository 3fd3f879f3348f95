"""Whole-frame numpy reference of the ray projections of a plane (DESIGN.md section
24).  Test infrastructure.

A ray is set up and stepped as ref_crossing._march steps it, but no opacity test is
made: every ray runs until t > tfar or 500 samples.  Its samples s_0 .. s_{n-1} --
blend(the 8 corner values, the footprint), ref_crossing.combine or .trilinear -- are
reduced in float32, one operation at a time, in step order:

    MAX   acc = -inf;  acc = s if s > acc else acc      (a NaN sample is skipped)
    MIN   acc = +inf;  acc = s if s < acc else acc
    MEAN  sum = 0;     sum = sum + s;  acc = sum / float32(n)

and the ray's value is classified once, x = (acc - toff) * tscale through the table
(ref_transfer.transfer_table; None: the built-in nine entries, ref_numpy.TF).  The
pixel is (r a, g a, b a, a) times brightness.  density is not an argument: a
projection has no steps to weigh.  The loop is restated here, not patched into
ref_crossing's.
"""
import numpy as np

import ref_crossing
import ref_numpy
from ref_numpy import _lin, pack
from ref_transfer import transfer_table

f32 = np.float32
MAX, MIN, MEAN = 1, 2, 3
MODES = {"max": MAX, "min": MIN, "mean": MEAN}


def reduce_init(mode):
    return f32(-np.inf) if mode == MAX else f32(np.inf) if mode == MIN else f32(0)


def reduce_step(mode, acc, s):
    """one sample into acc (arrays or scalars), float32"""
    if mode == MAX:
        return np.where(s > acc, s, acc).astype(np.float32)
    if mode == MIN:
        return np.where(s < acc, s, acc).astype(np.float32)
    return (acc + s).astype(np.float32)


def pixel(acc, table, brightness, toff, tscale):
    """acc (...) float32 -> saturated float RGBA (..., 4)"""
    col = transfer_table((acc - f32(toff)) * f32(tscale), ref_numpy.TF if table is None else table)
    a = col[..., 3]
    out = np.stack([col[..., 0] * a * f32(brightness), col[..., 1] * a * f32(brightness),
                    col[..., 2] * a * f32(brightness), a * f32(brightness)], -1)
    return np.where(out > 0, np.where(out > 1, f32(1), out), f32(0)).astype(np.float32)


def render_plane(F, W, H, m, mode, table=None, blend=ref_crossing.combine, brightness=1.0,
                 toff=0.0, tscale=1.0, info=None):
    """ref_crossing.render_plane's triple (packed RGBA8 (H, W) uint32, float RGBA
    (H, W, 4), samples per pixel (H, W), -1 = miss) of the projection `mode` (MAX, MIN,
    MEAN or their names) of the plane F (nz, ny, nx).  info: optional dict, receives
    acc (H, W) float32, the projected scalar (0 where the ray misses)."""
    mode = MODES.get(mode, mode)
    assert mode in (MAX, MIN, MEAN), mode
    with np.errstate(all="ignore"):
        return _march(np.asarray(F, dtype=np.float32), W, H, m, mode, table, blend, brightness,
                      toff, tscale, info)


def _march(F, W, H, m, mode, table, blend, brightness, toff, tscale, info):
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
    acc = np.full((H, W), reduce_init(mode), dtype=np.float32)
    n = np.where(hit, 0, -1)
    active = hit.copy()
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
        acc = np.where(active, reduce_step(mode, acc, sample), acc).astype(np.float32)
        n = np.where(active, i + 1, n)
        t = np.where(active, t + f32(0.01), t).astype(np.float32)
        active &= ~(t > tfar)
        pos = [np.where(active, pos[k] + step[k], pos[k]).astype(np.float32) for k in range(3)]
    if mode == MEAN:
        acc = np.where(hit, acc / np.maximum(n, 1).astype(np.float32), acc).astype(np.float32)
    out = pixel(acc, table, brightness, toff, tscale)
    out = np.where(hit[..., None], out, f32(0)).astype(np.float32)
    if info is not None:
        info.update(acc=np.where(hit, acc, f32(0)).astype(np.float32))
    return pack(out), out, n.astype(np.int32)


def render_ray(F, W, H, m, x, y, mode, table=None, blend=ref_crossing.combine, brightness=1.0,
               toff=0.0, tscale=1.0):
    """One pixel by a scalar loop: (float RGBA (4,), n, acc), or (None, -1, None) for a
    miss.  The same expressions as _march on numpy float32 scalars; tests hold the two
    against each other."""
    mode = MODES.get(mode, mode)
    F = np.asarray(F, dtype=np.float32)
    nz, ny, nx = F.shape
    M = np.asarray(m, dtype=np.float32).reshape(12)
    with np.errstate(all="ignore"):
        u = (f32(x) / f32(W)) * f32(2) - f32(1)
        v = (f32(y) / f32(H)) * f32(2) - f32(1)
        o = [f32(0) * M[4 * r] + f32(0) * M[4 * r + 1] + f32(0) * M[4 * r + 2] + f32(1) * M[4 * r + 3]
             for r in range(3)]
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
        if not tfar > tnear:
            return None, -1, None
        if tnear < 0:
            tnear = f32(0)
        pos = [f32(o[k] + d[k] * tnear) for k in range(3)]
        step = [f32(d[k] * f32(0.01)) for k in range(3)]
        t = f32(tnear)
        acc = reduce_init(mode)
        n = 0
        dims = (nx, ny, nz)
        for _ in range(500):
            ax = [_lin(np.asarray(pos[k] * f32(0.5) + f32(0.5), dtype=np.float32), dims[k])
                  for k in range(3)]
            vals = [F[ax[2][1 if j & 4 else 0], ax[1][1 if j & 2 else 0], ax[0][1 if j & 1 else 0]]
                    for j in range(8)]
            s = f32(blend(np.stack(vals), ax))
            if mode == MAX:
                acc = s if s > acc else acc
            elif mode == MIN:
                acc = s if s < acc else acc
            else:
                acc = f32(acc + s)
            n += 1
            t = f32(t + f32(0.01))
            if t > tfar:
                break
            pos = [f32(pos[k] + step[k]) for k in range(3)]
        if mode == MEAN:
            acc = f32(acc / f32(n))
        return pixel(np.asarray(acc, dtype=np.float32), table, brightness, toff, tscale), n, acc
