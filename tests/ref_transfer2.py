"""Whole-frame numpy reference of frames classified through a 2-D transfer function
over two planes of one volume.  Test infrastructure.

A table of nv x nu RGBA float32 entries (shape (nv, nu, 4): u fastest in memory) is
looked up bilinearly: ref_numpy._lin on each axis, ref_numpy._lerp along u in rows
j0 and j1, then along v, per channel, nothing in the table clamped.  The march is
ref_crossing._march restated for two planes (as ref_crossing restated ref_numpy):
the same ray set-up, step, compositing, info dict and return triple, with one
footprint per step serving both planes.
"""
import numpy as np

import ref_crossing
from ref_numpy import _lerp, _lin, pack

f32 = np.float32


def transfer_table2(xu, xv, table):
    """xu, xv (...) -> RGBA (..., 4) float32 of the (nv, nu, 4) table at the
    normalised coordinates (each clamped to [0, 1], NaN as 0)"""
    t = np.asarray(table, dtype=np.float32)
    assert t.ndim == 3 and t.shape[2] == 4, t.shape
    nv, nu = t.shape[:2]
    assert 1 <= nu <= 256 and 1 <= nv <= 256 and nu * nv <= 1024, t.shape
    xu, xv = np.broadcast_arrays(np.asarray(xu, dtype=np.float32),
                                 np.asarray(xv, dtype=np.float32))
    with np.errstate(all="ignore"):
        i0, i1, a = _lin(xu, nu)
        j0, j1, b = _lin(xv, nv)
        r0 = _lerp(t[j0, i0], t[j0, i1], a[..., None])
        r1 = _lerp(t[j1, i0], t[j1, i1], a[..., None])
        return _lerp(r0, r1, b[..., None]).astype(np.float32)


def render_planes(Fu, Fv, W, H, m, table, blend_u=ref_crossing.trilinear,
                  blend_v=ref_crossing.trilinear, voff=0.0, vscale=1.0, density=0.05,
                  brightness=1.0, toff=0.0, tscale=1.0, info=None):
    """ref_crossing.render_plane's triple (RGBA8, float RGBA, samples per pixel) of a
    frame marched over the planes Fu and Fv (nz, ny, nx) of one volume: at each
    sample su = blend_u(Fu's 8 corners), sv = blend_v(Fv's), classified through
    `table` at ((su - toff) * tscale, (sv - voff) * vscale).  blend_*:
    ref_crossing.combine (method 13) or ref_crossing.trilinear.  info: as there."""
    Fu, Fv = np.asarray(Fu, dtype=np.float32), np.asarray(Fv, dtype=np.float32)
    assert Fu.shape == Fv.shape and Fu.ndim == 3, (Fu.shape, Fv.shape)
    with np.errstate(all="ignore"):
        return _march(Fu, Fv, W, H, m, table, blend_u, blend_v, voff, vscale, density, brightness,
                      toff, tscale, info)


def _march(Fu, Fv, W, H, m, table, blend_u, blend_v, voff, vscale, density, brightness, toff,
           tscale, info):
    nz, ny, nx = Fu.shape
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
        vu, vv = [], []
        for j in range(8):
            xi = ax[0][1] if j & 1 else ax[0][0]
            yi = ax[1][1] if j & 2 else ax[1][0]
            zi = ax[2][1] if j & 4 else ax[2][0]
            vu.append(Fu[zi, yi, xi])
            vv.append(Fv[zi, yi, xi])
        su = blend_u(np.stack(vu), ax)
        sv = blend_v(np.stack(vv), ax)
        edge = (ax[0][0] == ax[0][1]) | (ax[1][0] == ax[1][1]) | (ax[2][0] == ax[2][1])
        samples += int(active.sum())
        clamped += int((active & edge).sum())
        col = transfer_table2((su - f32(toff)) * f32(tscale), (sv - f32(voff)) * f32(vscale),
                              table)
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
