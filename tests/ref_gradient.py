"""numpy float32 restatement of the gradient-magnitude planes (DESIGN.md section
26.1).  Test infrastructure.

For a plane s (nz, ny, nx) of one float per voxel, at every voxel, one float32
operation at a time:

    xm = x > 0 ? x - 1 : 0          xp = x + 1 < nx ? x + 1 : nx - 1        (y, z alike)
    dx = s(xp, y, z) - s(xm, y, z)
    hx = (xp - xm == 2) ? (float)nx * 0.5f : (float)nx
    Gx = dx * hx                    Gy, Gz alike with ny, nz
    m  = sqrtf((Gx * Gx + Gy * Gy) + Gz * Gz)

gradient_plane is the array form, gradient_voxel / gradient_plane_scalar the scalar
loop per voxel; tests/test_gradient.py holds each to the other bit for bit.  The
maximum is the unsigned maximum of the bit patterns (m is never negative).

MUTANTS names three wrong versions of the arithmetic that the tests must be able to
tell from the right one (test_gradient.py's census): a forward difference instead of
the central one, no n factors, and faces set to 0 instead of the one-sided
difference.  Frames of a gradient plane come from the existing renderers
(ref_transfer, ref_transfer2, ref_projection, ref_shading) fed the plane.
"""
import numpy as np

f32 = np.float32
MUTANTS = ("forward", "no_n", "zero_faces")


def _neighbours(n, mutant):
    """(minus index, plus index, spacing factor float32) of every index of an axis"""
    i = np.arange(n)
    m, p = np.maximum(i - 1, 0), np.minimum(i + 1, n - 1)
    central = p - m == 2
    if mutant == "forward":
        m, central = i, np.zeros(n, bool)
    nn = f32(1) if mutant == "no_n" else f32(n)
    h = np.where(central, nn * f32(0.5), nn).astype(np.float32)
    if mutant == "zero_faces":
        h = np.where(central, h, f32(0)).astype(np.float32)
    return m, p, h


def gradient_plane(F, mutant=None):
    """(|grad F| (nz, ny, nx) float32, its maximum float32), the array form"""
    F = np.asarray(F, dtype=np.float32)
    assert F.ndim == 3 and mutant in (None,) + MUTANTS
    G = []
    for axis in (2, 1, 0):  # x, y, z
        m, p, h = _neighbours(F.shape[axis], mutant)
        shape = [1, 1, 1]
        shape[axis] = -1
        d = (np.take(F, p, axis=axis) - np.take(F, m, axis=axis)).astype(np.float32)
        G.append((d * h.reshape(shape)).astype(np.float32))
    gx, gy, gz = G
    mag = np.sqrt(((gx * gx + gy * gy).astype(np.float32) + gz * gz).astype(np.float32))
    mag = np.ascontiguousarray(mag, dtype=np.float32)
    return mag, bits_max(mag)


def bits_max(mag):
    """the maximum of non-negative floats as the unsigned maximum of their bits"""
    return np.array([mag.view(np.uint32).max()], np.uint32).view(np.float32)[0]


def gradient_voxel(F, x, y, z):
    """|grad F| at one voxel, the scalar loop of section 26.1"""
    nz, ny, nx = F.shape
    G = []
    for c, n, at in ((x, nx, lambda i: F[z, y, i]), (y, ny, lambda i: F[z, i, x]),
                     (z, nz, lambda i: F[i, y, x])):
        cm = c - 1 if c > 0 else 0
        cp = c + 1 if c + 1 < n else n - 1
        d = f32(f32(at(cp)) - f32(at(cm)))
        h = f32(f32(n) * f32(0.5)) if cp - cm == 2 else f32(n)
        G.append(f32(d * h))
    gx, gy, gz = G
    return np.sqrt(f32(f32(f32(gx * gx) + f32(gy * gy)) + f32(gz * gz)))


def gradient_plane_scalar(F):
    """gradient_plane's pair, voxel by voxel"""
    F = np.asarray(F, dtype=np.float32)
    nz, ny, nx = F.shape
    out = np.zeros(F.shape, np.float32)
    best = 0
    with np.errstate(all="ignore"):
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    out[z, y, x] = gradient_voxel(F, x, y, z)
                    best = max(best, int(out[z, y, x].view(np.uint32)))
    return out, np.array([best], np.uint32).view(np.float32)[0]
