"""Whole-frame numpy reference of headlight gradient shading of a plane (DESIGN.md
section 25.1).  Test infrastructure.

A ray is set up, stepped and ended exactly as ref_crossing._march does it.  At each
sample the 8 corner values s0..s7 (gather order: x = j & 1, y = j & 2, z = j & 4), the
footprint weights ax, ay, az and the ray direction (dx, dy, dz) give, in float32, one
operation at a time:

    c00 = lerp(s0, s1, ax)  c10 = lerp(s2, s3, ax)  c01 = lerp(s4, s5, ax)  c11 = lerp(s6, s7, ax)
    c0  = lerp(c00, c10, ay)  c1 = lerp(c01, c11, ay)
    gx  = lerp(lerp(s1 - s0, s3 - s2, ay), lerp(s5 - s4, s7 - s6, ay), az)
    gy  = lerp(c10 - c00, c11 - c01, az)
    gz  = c1 - c0
    Gx = gx * nx   Gy = gy * ny   Gz = gz * nz
    g2 = (Gx * Gx + Gy * Gy) + Gz * Gz
    gd = (Gx * dx + Gy * dy) + Gz * dz
    c  = |gd| / sqrt(g2) if g2 > 0 else 1;   c = c if c < 1 else 1     (a NaN becomes 1)
    p  = c;  k times: p = p * p
    shade = ka + kd * c     spec = ks * p

The sample is blend(s, footprint) as ever; the table's colour becomes col * shade +
spec per colour channel before it is weighted by its opacity; alpha is untouched.  The
loop is restated here, not patched into ref_crossing's.  light = (ka, kd, ks, k).
"""
import numpy as np

import ref_crossing
import ref_numpy
from ref_numpy import _lerp, _lin, pack
from ref_transfer import transfer_table

f32 = np.float32
IDENTITY = (1.0, 0.0, 0.0, 0)


MUTANTS = ("unscaled", "lit_alpha")


def gradient(vals, ax, dims):
    """vals (8, ...) float32 corner values, ax the three _lin results (i0, i1, a) of
    x, y, z, dims (nx, ny, nz) -> (Gx, Gy, Gz): the gradient of the trilinear
    interpolant inside the cell, per unit of the normalised volume"""
    s = np.asarray(vals, dtype=np.float32)
    a, b, c = ax[0][2], ax[1][2], ax[2][2]
    with np.errstate(all="ignore"):
        c00 = _lerp(s[0], s[1], a)
        c10 = _lerp(s[2], s[3], a)
        c01 = _lerp(s[4], s[5], a)
        c11 = _lerp(s[6], s[7], a)
        c0 = _lerp(c00, c10, b)
        c1 = _lerp(c01, c11, b)
        gx = _lerp(_lerp(s[1] - s[0], s[3] - s[2], b), _lerp(s[5] - s[4], s[7] - s[6], b), c)
        gy = _lerp(c10 - c00, c11 - c01, c)
        gz = c1 - c0
        return ((gx * f32(dims[0])).astype(np.float32), (gy * f32(dims[1])).astype(np.float32),
                (gz * f32(dims[2])).astype(np.float32))


def cosine(G, d):
    """G the gradient, d the three ray-direction components -> c in [0, 1] float32"""
    with np.errstate(all="ignore"):
        g2 = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]
        gd = (G[0] * d[0] + G[1] * d[1]) + G[2] * d[2]
        c = np.where(g2 > 0, np.abs(gd) / np.sqrt(g2), f32(1)).astype(np.float32)
        return np.where(c < 1, c, f32(1)).astype(np.float32)


def shade(c, light):
    """c -> (shade, spec) float32 under light = (ka, kd, ks, k)"""
    ka, kd, ks, k = light
    with np.errstate(all="ignore"):
        c = np.asarray(c, dtype=np.float32)
        p = c
        for _ in range(int(k)):
            p = p * p
        return (f32(ka) + f32(kd) * c).astype(np.float32), (f32(ks) * p).astype(np.float32)


def render_plane(F, W, H, m, table, light, blend=ref_crossing.combine, density=0.05,
                 brightness=1.0, toff=0.0, tscale=1.0, info=None, mutant=None):
    """ref_crossing.render_plane's triple (packed RGBA8 (H, W) uint32, float RGBA
    (H, W, 4), samples per pixel (H, W), -1 = miss) of the plane F (nz, ny, nx) lit by
    `light`, classified through `table` (None: the built-in nine entries).  info:
    optional dict, receives samples (taken), clamped (taken in a cell whose footprint
    the volume's edge clamps along an axis), flat (taken where g2 > 0 is false) and c
    (a float32 array of every sample's cosine, in no particular order).  mutant: one of
    MUTANTS, a wrong version a census must be able to tell from the right one (the
    gradient not scaled by the dims; alpha lit as the colours are)."""
    assert mutant in (None,) + MUTANTS
    with np.errstate(all="ignore"):
        return _march(np.asarray(F, dtype=np.float32), W, H, m,
                      ref_numpy.TF if table is None else table, light, blend, density, brightness,
                      toff, tscale, info, mutant)


def _march(F, W, H, m, table, light, blend, density, brightness, toff, tscale, info, mutant=None):
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
    samples = flat = clamped = 0
    cs = []
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
        vals = np.stack(vals)
        sample = blend(vals, ax)
        G = gradient(vals, ax, (1, 1, 1) if mutant == "unscaled" else dims)
        c = cosine(G, d)
        sh, sp = shade(c, light)
        if info is not None:
            g2 = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]
            edge = (ax[0][0] == ax[0][1]) | (ax[1][0] == ax[1][1]) | (ax[2][0] == ax[2][1])
            samples += int(active.sum())
            clamped += int((active & edge).sum())
            flat += int((active & ~(g2 > 0)).sum())
            cs.append(c[active])
        col = transfer_table((sample - f32(toff)) * f32(tscale), table)
        rgb = [col[..., k] * sh + sp for k in range(3)]
        alpha = col[..., 3] * sh + sp if mutant == "lit_alpha" else col[..., 3]
        cw = alpha * f32(density)
        col = np.stack([rgb[0] * cw, rgb[1] * cw, rgb[2] * cw, cw], -1)
        om = f32(1) - s[..., 3]
        ns = s + col * om[..., None]
        s = np.where(active[..., None], ns, s)
        n = np.where(active, i + 1, n)
        done = s[..., 3] > f32(0.95)
        t = np.where(active & ~done, t + f32(0.01), t).astype(np.float32)
        done |= t > tfar
        active &= ~done
        pos = [np.where(active, pos[k] + step[k], pos[k]).astype(np.float32) for k in range(3)]
    out = s * f32(brightness)
    out = np.where(out > 0, np.where(out > 1, f32(1), out), f32(0))
    out = np.where(hit[..., None], out, f32(0)).astype(np.float32)
    if info is not None:
        info.update(samples=samples, flat=flat, clamped=clamped,
                    c=np.concatenate(cs) if cs else np.zeros(0, np.float32))
    return pack(out), out, n.astype(np.int32)


def render_ray(F, W, H, m, x, y, table, light, blend=ref_crossing.combine, density=0.05,
               brightness=1.0, toff=0.0, tscale=1.0):
    """One pixel by a scalar loop: (float RGBA (4,), n), or (None, -1) for a miss.  The
    expressions of section 25.1 written out on numpy float32 scalars, the blend and the
    table's classifier called per sample; tests hold it against _march."""
    F = np.asarray(F, dtype=np.float32)
    table = ref_numpy.TF if table is None else table
    nz, ny, nx = F.shape
    ka, kd, ks, k = f32(light[0]), f32(light[1]), f32(light[2]), int(light[3])
    M = np.asarray(m, dtype=np.float32).reshape(12)
    lerp = lambda a, b, w: f32(f32((f32(1) - w) * a) + f32(w * b))
    with np.errstate(all="ignore"):
        u = (f32(x) / f32(W)) * f32(2) - f32(1)
        v = (f32(y) / f32(H)) * f32(2) - f32(1)
        o = [f32(0) * M[4 * r] + f32(0) * M[4 * r + 1] + f32(0) * M[4 * r + 2] + f32(1) * M[4 * r + 3]
             for r in range(3)]
        inv = f32(1) / np.sqrt(u * u + v * v + f32(-2) * f32(-2))
        d0 = [u * inv, v * inv, f32(-2) * inv]
        d = [d0[0] * M[4 * r] + d0[1] * M[4 * r + 1] + d0[2] * M[4 * r + 2] for r in range(3)]
        invR = [f32(1) / d[j] for j in range(3)]
        tb = [invR[j] * (f32(-1) - o[j]) for j in range(3)]
        tt = [invR[j] * (f32(1) - o[j]) for j in range(3)]
        tmn = [np.fmin(tt[j], tb[j]) for j in range(3)]
        tmx = [np.fmax(tt[j], tb[j]) for j in range(3)]
        tnear = np.fmax(np.fmax(tmn[0], tmn[1]), np.fmax(tmn[0], tmn[2]))
        tfar = np.fmin(np.fmin(tmx[0], tmx[1]), np.fmin(tmx[0], tmx[2]))
        if not tfar > tnear:
            return None, -1
        if tnear < 0:
            tnear = f32(0)
        pos = [f32(o[j] + d[j] * tnear) for j in range(3)]
        step = [f32(d[j] * f32(0.01)) for j in range(3)]
        t = f32(tnear)
        acc = [f32(0)] * 4
        n = 0
        dims = (nx, ny, nz)
        for _ in range(500):
            ax = [_lin(np.asarray(pos[j] * f32(0.5) + f32(0.5), dtype=np.float32), dims[j])
                  for j in range(3)]
            s = [f32(F[ax[2][1 if j & 4 else 0], ax[1][1 if j & 2 else 0], ax[0][1 if j & 1 else 0]])
                 for j in range(8)]
            a, b, c_ = f32(ax[0][2]), f32(ax[1][2]), f32(ax[2][2])
            c00, c10 = lerp(s[0], s[1], a), lerp(s[2], s[3], a)
            c01, c11 = lerp(s[4], s[5], a), lerp(s[6], s[7], a)
            c0, c1 = lerp(c00, c10, b), lerp(c01, c11, b)
            gx = lerp(lerp(f32(s[1] - s[0]), f32(s[3] - s[2]), b),
                      lerp(f32(s[5] - s[4]), f32(s[7] - s[6]), b), c_)
            gy = lerp(f32(c10 - c00), f32(c11 - c01), c_)
            gz = f32(c1 - c0)
            Gx, Gy, Gz = f32(gx * f32(nx)), f32(gy * f32(ny)), f32(gz * f32(nz))
            g2 = f32(f32(f32(Gx * Gx) + f32(Gy * Gy)) + f32(Gz * Gz))
            gd = f32(f32(f32(Gx * d[0]) + f32(Gy * d[1])) + f32(Gz * d[2]))
            c = f32(np.abs(gd) / np.sqrt(g2)) if g2 > 0 else f32(1)
            c = c if c < 1 else f32(1)
            p = c
            for _k in range(k):
                p = f32(p * p)
            sh, sp = f32(ka + f32(kd * c)), f32(ks * p)
            sample = f32(blend(np.stack(s), ax))
            col = transfer_table(np.asarray((sample - f32(toff)) * f32(tscale), dtype=np.float32),
                                 table)
            rgb = [f32(f32(col[j] * sh) + sp) for j in range(3)]
            cw = f32(col[3] * f32(density))
            col = [f32(rgb[0] * cw), f32(rgb[1] * cw), f32(rgb[2] * cw), cw]
            om = f32(f32(1) - acc[3])
            acc = [f32(acc[j] + f32(col[j] * om)) for j in range(4)]
            n += 1
            if acc[3] > f32(0.95):
                break
            t = f32(t + f32(0.01))
            if t > tfar:
                break
            pos = [f32(pos[j] + step[j]) for j in range(3)]
        out = np.array([f32(a * f32(brightness)) for a in acc], dtype=np.float32)
        out = np.where(out > 0, np.where(out > 1, f32(1), out), f32(0)).astype(np.float32)
        return out, n
