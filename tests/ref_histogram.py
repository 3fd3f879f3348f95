"""numpy restatement of the value ranges and histograms of baked planes (DESIGN.md
section 27.1).  Test infrastructure.

The bin of plane value s under the window (offset, scale) of an axis of n entries,
float32, one operation at a time:

    x = (s - offset) * scale
    u = fmin(fmax(x, 0), 1)                  (a NaN gives 0)
    i = min((int)floor(u * (float)n), n - 1)

counts[j * nu + i] is the number of voxels of the box whose u plane has bin i and
whose v plane has bin j; the range is the minimum and maximum by the monotone key of
the bit pattern (bits ^ 0x80000000 for a non-negative pattern, ~bits for a negative
one: -0 < +0) over the voxels that are not NaN, NaN if there is none, and the number
that are.  histogram / plane_range are the array forms, histogram_scalar /
plane_range_scalar the loops per voxel; tests/test_histogram.py holds each to the
other.  Planes are (nz, ny, nx) arrays, a box is (x0, x1, y0, y1, z0, z1) or None.

MUTANTS names five wrong versions the tests must be able to tell from the right one:
the apron copies of the brick layout counted as voxels (x = 15 k, k > 0, twice), the
empty slots of the layout counted (+0 in both planes), the nearest table entry
(floor(x n - 0.5)) instead of the cell, u and v exchanged, and values outside the
window dropped instead of clamped into the edge bins.
"""
import numpy as np

f32 = np.float32
MUTANTS = ("aprons", "empty_slots", "nearest", "swapped", "dropped")
NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def coordinate(s, offset, scale):
    """x = (s - offset) * scale in float32"""
    with np.errstate(all="ignore"):
        d = (np.asarray(s, np.float32) - f32(offset)).astype(np.float32)
        return (d * f32(scale)).astype(np.float32)


def bin_of(s, offset, scale, n, mutant=None):
    """the bins of the values s (any shape), int64"""
    x = coordinate(s, offset, scale)
    with np.errstate(all="ignore"):
        u = np.fmin(np.fmax(x, f32(0)), f32(1)).astype(np.float32)
        t = (u * f32(n)).astype(np.float32)
        if mutant == "nearest":
            t = (t - f32(0.5)).astype(np.float32)
        i = np.floor(t).astype(np.int64)
    return np.clip(i, 0, n - 1) if mutant == "nearest" else np.minimum(i, n - 1)


def crop(plane, box):
    plane = np.asarray(plane, np.float32)
    assert plane.ndim == 3
    if box is None:
        return plane
    x0, x1, y0, y1, z0, z1 = box
    return plane[z0:z1, y0:y1, x0:x1]


def _extra_slots(shape, box, mutant):
    """how often a mutant counts beyond the voxels: (weights per voxel, empty slots)"""
    nz, ny, nx = shape
    x0, x1, y0, y1, z0, z1 = box if box is not None else (0, nx, 0, ny, 0, nz)
    w = np.ones((z1 - z0, y1 - y0, x1 - x0), np.int64)
    empty = 0
    if mutant == "aprons":  # x = 15 k, k > 0, is stored in brick k - 1 as well
        xs = np.arange(x0, x1)
        w[:, :, (xs > 0) & (xs % 15 == 0)] += 1
    if mutant == "empty_slots":  # slots of the bricks the box meets that hold no voxel
        kx0, kx1 = x0 // 15, (x1 - 1) // 15
        yp0, yp1 = y0 // 2, (y1 - 1) // 2
        for kx in range(kx0, kx1 + 1):
            cols = sum(1 for o in range(16) if 15 * kx + o >= nx)
            rows_all = 2 * (yp1 - yp0 + 1)
            rows_out = sum(1 for y in range(2 * yp0, 2 * yp1 + 2) if y >= ny)
            empty += cols * rows_all + (16 - cols) * rows_out
        empty *= z1 - z0
    return w, empty


def histogram(pu, nu, wu, pv=None, nv=1, wv=(0.0, 1.0), box=None, mutant=None):
    """counts (nv, nu) uint64 of the voxels of box, the array form"""
    assert mutant in (None,) + MUTANTS
    pu = np.asarray(pu, np.float32)
    if pv is None:
        assert nv == 1
    su = crop(pu, box)
    sv = crop(pv, box) if pv is not None else None
    if mutant == "swapped" and sv is not None:
        su, sv = sv, su
    i = bin_of(su, wu[0], wu[1], nu, mutant)
    j = bin_of(sv, wv[0], wv[1], nv, mutant) if sv is not None else np.zeros_like(i)
    w, empty = _extra_slots(pu.shape, box, mutant)
    if mutant == "dropped":
        with np.errstate(all="ignore"):
            xu = coordinate(su, wu[0], wu[1])
            keep = (xu >= 0) & (xu <= 1)
            if sv is not None:
                xv = coordinate(sv, wv[0], wv[1])
                keep &= (xv >= 0) & (xv <= 1)
        w = w * keep
    counts = np.bincount((j * nu + i).ravel(), weights=None if mutant is None else w.ravel(),
                         minlength=nu * nv).astype(np.uint64)
    if empty:  # +0 in every plane
        i0 = int(bin_of(f32(0), wu[0], wu[1], nu))
        j0 = int(bin_of(f32(0), wv[0], wv[1], nv)) if sv is not None else 0
        counts[j0 * nu + i0] += np.uint64(empty)
    return counts.reshape(nv, nu)


def histogram_scalar(pu, nu, wu, pv=None, nv=1, wv=(0.0, 1.0), box=None):
    """histogram's counts, voxel by voxel with Python's own floor and comparisons"""
    import math
    pu = np.asarray(pu, np.float32)
    nz, ny, nx = pu.shape
    x0, x1, y0, y1, z0, z1 = box if box is not None else (0, nx, 0, ny, 0, nz)

    def one(s, off, scale, n):
        with np.errstate(all="ignore"):
            x = f32(f32(f32(s) - f32(off)) * f32(scale))
        if not x > 0:  # NaN, -0, +0 and below
            x = f32(0)
        if x > 1:
            x = f32(1)
        return min(int(math.floor(float(f32(x * f32(n))))), n - 1)

    counts = [0] * (nu * nv)
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                i = one(pu[z, y, x], wu[0], wu[1], nu)
                j = one(pv[z, y, x], wv[0], wv[1], nv) if pv is not None else 0
                counts[j * nu + i] += 1
    return np.array(counts, np.uint64).reshape(nv, nu)


def keys(bits):
    """the monotone keys of float32 bit patterns (uint32 in, uint32 out)"""
    bits = np.asarray(bits, np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits ^ np.uint32(0x80000000))


def unkey(k):
    k = np.uint32(k)
    b = k ^ np.uint32(0x80000000) if k & np.uint32(0x80000000) else ~k
    return np.array([b], np.uint32).view(np.float32)[0]


def plane_range(plane, box=None):
    """(min, max, n_nan): float32, float32, int, the array form"""
    s = np.ascontiguousarray(crop(plane, box), dtype=np.float32)
    nan = np.isnan(s)
    n_nan = int(nan.sum())
    if n_nan == s.size:
        return NAN, NAN, n_nan
    k = keys(s.view(np.uint32)[~nan])
    return unkey(k.min()), unkey(k.max()), n_nan


def plane_range_scalar(plane, box=None):
    """plane_range's triple, voxel by voxel"""
    s = np.ascontiguousarray(crop(plane, box), dtype=np.float32)
    lo, hi, n_nan = None, None, 0
    for b in s.view(np.uint32).ravel().tolist():
        if (b & 0x7FFFFFFF) > 0x7F800000:
            n_nan += 1
            continue
        k = (~b & 0xFFFFFFFF) if b & 0x80000000 else b ^ 0x80000000
        lo = k if lo is None else min(lo, k)
        hi = k if hi is None else max(hi, k)
    if lo is None:
        return NAN, NAN, n_nan
    return unkey(lo), unkey(hi), n_nan


def window(plane, box=None):
    """api.plane_window: (min, float32(1) / (max - min)), scale 1.0 when max <= min"""
    lo, hi, _ = plane_range(plane, box)
    if not hi > lo:
        return float(lo), 1.0
    with np.errstate(all="ignore"):
        return float(lo), float(f32(1) / f32(hi - lo))
