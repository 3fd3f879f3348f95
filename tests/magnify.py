"""Decode-magnifying scenes: the scene table and helpers of the bit-parity tests.

The transfer function quantises its coordinate to 8 fractional bits over 9
texels, so at transfer_scale = 1 a statistic that is wrong in its last bit
changes a frame only where a sample crosses one of 9 x 256 levels: almost
never.  A scene here renders the same volume through
one to seven narrow transfer windows (transfer_scale 256 or 1024, the
offset stepped across the statistic's range), where a 1-ulp change of one
corner's statistic moves pixels; frames are then compared word for word.

tests/test_magnified_scenes.py proves the sensitivity of every scene on the
CPU with the oracle's statistic nudge (PINNED below);
tests/test_gpu_bitparity.py holds the GPU marches to the oracle on them.

CPU only.  Nothing in this module accepts a difference.
"""
import collections
import ctypes
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402

DIMS = (26, 22, 18)
M7_GRID = (10, 12, 20)  # a method-7 grid that is not the volume's

# kind: "hist" (methods 1/2/3/7), "codec" (4/5/6), "gmm" (1/2); size: bins or K;
# grid: method 7's corner grid; f16: the records rounded to float16 and widened;
# W x H: the frame (80 x 64; smaller where an oracle sample is dear: wide
# records, codec voxels, GMM records)
Scene = collections.namedtuple(
    "Scene", "name kind size method cam f16 grid W H density tscale nwin")

FRAME = {("hist", 16): (64, 48), ("hist", 32): (60, 40), ("codec", 8): (56, 40),
         ("codec", 32): (56, 40), ("gmm", 8): (64, 48), ("gmm", 16): (64, 48),
         ("gmm", 32): (48, 40)}

# windows per scene: the fewest, from 1 up, with which every corner and either
# sign changes at least MIN_LIT pixels (found with the oracle alone,
# tests/test_magnified_scenes.py); a scene not listed takes 4
NWIN = {
    "hist4-m1-C0": 1, "hist4-m2-C0": 1, "hist4-m3-C0": 1, "hist4-m1-OBL": 1, "hist4-m2-OBL": 1,
    "hist4-m3-OBL": 1, "hist8-m1-C0": 1, "hist8-m2-C0": 1, "hist8-m3-C0": 1, "hist8-m1-OBL": 1,
    "hist8-m2-OBL": 1, "hist8-m3-OBL": 1, "hist8-m1-SIDE": 1, "hist8-m2-SIDE": 2,
    "hist8-m3-SIDE": 1, "hist1-m2-C0": 7, "hist1-m1-OBL": 5, "hist1-m2-OBL": 5,
    "hist2-m1-C0": 1, "hist2-m2-C0": 1, "hist2-m3-C0": 3, "hist2-m1-OBL": 1, "hist2-m2-OBL": 1,
    "hist3-m1-C0": 1, "hist3-m2-C0": 2, "hist3-m3-C0": 2, "hist5-m1-OBL": 1, "hist5-m2-OBL": 3,
    "hist5-m3-OBL": 1, "hist16-m1-C0": 1, "hist16-m2-C0": 1, "hist16-m3-C0": 1,
    "hist16-m1-OBL": 1, "hist16-m2-OBL": 1, "hist16-m3-OBL": 1, "hist32-m1-C0": 1,
    "hist32-m2-C0": 1, "hist32-m3-C0": 1, "hist32-m1-OBL": 1, "hist32-m2-OBL": 1,
    "hist32-m3-OBL": 1, "hist8-m7-C0-g26x22x18": 1, "hist8-m7-OBL-g26x22x18": 1,
    "hist8-m7-SIDE-g26x22x18": 1, "hist8-m7-OBL-g10x12x20": 1, "codec8-m5-C0": 7,
    "codec8-m6-C0": 3, "codec8-m4-OBL": 3, "codec8-m5-OBL": 7, "codec8-m6-OBL": 3,
    "codec32-m4-OBL": 3, "codec32-m5-OBL": 5, "codec32-m6-OBL": 1, "gmm8-m1-OBL": 1,
    "gmm8h-m1-C0": 1, "gmm8-m2-OBL": 3, "gmm8h-m2-C0": 3, "gmm16-m1-OBL": 1, "gmm16h-m1-C0": 1,
    "gmm16-m2-OBL": 1, "gmm16h-m2-C0": 1, "gmm32-m1-OBL": 2, "gmm32h-m1-C0": 1,
    "gmm32-m2-OBL": 1, "gmm32h-m2-C0": 1, "hist1h-m2-OBL": 7, "hist8h-m1-OBL": 1,
    "hist8h-m2-OBL": 1, "hist8h-m3-OBL": 1, "hist32h-m1-OBL": 1, "hist32h-m2-OBL": 2,
    "hist32h-m3-OBL": 1,
}

_camera_mod = None


def camera(cam):
    """C0: the reference's single-test view; OBL: the (30, 45) oblique view;
    SIDE: the (-60, 110) side view -- the three of test_every_kernel_path"""
    global _camera_mod
    if _camera_mod is None:
        spec = importlib.util.spec_from_file_location(
            "vr_camera", os.path.join(ROOT, "volume-rendering-based-on-distribution-data_amd",
                                      "camera.py"))
        _camera_mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_camera_mod)
    if cam == "C0":
        return _camera_mod.single_test_inv_view()
    return _camera_mod.display_inv_view({"OBL": (30.0, 45.0), "SIDE": (-60.0, 110.0)}[cam])


def _scenes():
    out = []

    def add(kind, size, method, cam, f16=False, grid=None):
        name = f"{kind}{size}{'h' if f16 else ''}-m{method}-{cam}"
        if grid:
            name += "-g%dx%dx%d" % grid
        w, h = FRAME.get((kind, size), (80, 64))
        # (the codec variance spreads thinly over a wide range: narrower windows)
        kw = dict(density=0.5, tscale=1024.0 if (kind, method) == ("codec", 5) else 256.0,
                  nwin=NWIN.get(name, 4))
        out.append(Scene(name, kind, size, method, cam, f16, grid, w, h, **kw))

    def methods(nb):
        return (1, 2, 3) if nb > 1 else (1, 2)  # the entropy of one bin is constant

    for nb, cams in ((4, ("C0", "OBL")), (8, ("C0", "OBL", "SIDE"))):
        for cam in cams:
            for method in (1, 2, 3):
                add("hist", nb, method, cam)
    # (3 and 5 bins share the runtime-B kernels: one camera each)
    for nb, cams in ((1, ("C0", "OBL")), (2, ("C0", "OBL")), (3, ("C0",)), (5, ("OBL",)),
                     (16, ("C0", "OBL")), (32, ("C0", "OBL"))):
        for cam in cams:
            for method in methods(nb):
                add("hist", nb, method, cam)
    for cam, grid in (("C0", DIMS), ("OBL", DIMS), ("SIDE", DIMS), ("OBL", M7_GRID)):
        add("hist", 8, 7, cam, grid=grid)
    for nb, cams in ((8, ("C0", "OBL")), (32, ("OBL",))):
        for cam in cams:
            for method in (4, 5, 6):
                add("codec", nb, method, cam)
    for K in (8, 16, 32):
        for method in (1, 2):
            add("gmm", K, method, "OBL")
            add("gmm", K, method, "C0", f16=True)
    for nb in (1, 8, 32):
        for method in methods(nb):
            add("hist", nb, method, "OBL", f16=True)
    return out


SCENES = _scenes()
BY_NAME = {s.name: s for s in SCENES}
assert len(BY_NAME) == len(SCENES)


def select(kind, sizes=None, methods=None, f16=False, cams=None, grid="any"):
    return [s for s in SCENES
            if s.kind == kind and s.f16 == f16 and (sizes is None or s.size in sizes)
            and (methods is None or s.method in methods) and (cams is None or s.cam in cams)
            and (grid == "any" or s.grid == grid)]


# ---- volumes, statistic ranges and windows ----

_volumes = {}
_ranges = {}


def orc():
    return graft.load_oracle()


def _total(a):
    """sum over the last axis, one element-wise add per entry: the same bits on
    every numpy build (a library reduction may pick its own order)"""
    t = np.zeros(a.shape[:-1] + (1,))
    for k in range(a.shape[-1]):
        t[..., 0] += a[..., k]
    return t


def _random_hist(nb):
    """every voxel its own random histogram (numpy PCG64, seeded): the statistics
    vary from voxel to voxel, so the samples of a frame spread over the
    statistic's range and every window shows many; a tenth of the bins are
    exactly 0 (the entropy's pr <= 0 branch)"""
    rng = np.random.default_rng(1000 + nb)
    nx, ny, nz = DIMS
    p = rng.random((nz, ny, nx, nb))
    p = p * p * p  # spiky histograms
    if nb > 1:
        p[rng.random(p.shape) < 0.1] = 0.0
        p[..., 0] += 1e-3
        p /= _total(p)
    return np.ascontiguousarray(p.astype(np.float32))


def _random_gmm(K):
    """every voxel its own random mixture: weights summing to 1, means in [0, 1],
    sigmas in [0.005, 0.055] (the generator's range)"""
    rng = np.random.default_rng(2000 + K)
    nx, ny, nz = DIMS
    w = rng.random((nz, ny, nx, K)) + 0.05
    w /= _total(w)
    wm = np.stack([w, rng.random(w.shape)], axis=-1).astype(np.float32)
    sg = (0.005 + 0.05 * rng.random(w.shape)).astype(np.float32)
    return np.ascontiguousarray(wm), np.ascontiguousarray(sg)


def volume(scene):
    """the scene's records as the oracle takes them (float32; f16 scenes: rounded
    to float16 and widened, exact), cached and read-only:
    hist: (nz, ny, nx, B); codec: (codebook, templates, errors); gmm: (wm, sg)"""
    key = (scene.kind, scene.size, scene.f16)
    if key not in _volumes:
        if scene.kind == "hist":
            v = (_random_hist(scene.size),)
        elif scene.kind == "codec":
            v = orc().synth_codec(*DIMS, scene.size, seed=scene.size)
        else:
            v = _random_gmm(scene.size)
        if scene.f16:
            v = tuple(a.astype(np.float16).astype(np.float32) for a in v)
        for a in v:
            a.setflags(write=False)
        _volumes[key] = v[0] if scene.kind == "hist" else v
    return _volumes[key]


def volume_f16(scene):
    """what an f16 scene uploads: the same records as float16"""
    assert scene.f16
    v = volume(scene)
    if scene.kind == "hist":
        return v.astype(np.float16)
    return tuple(a.astype(np.float16) for a in v)


def _p10_p90(v):
    q = np.sort(v)
    return float(q[len(q) // 10]), float(q[len(q) - 1 - len(q) // 10])


def stat_range(scene):
    """(lo, hi) of the statistic the scene's method samples: the 10th and 90th
    percentile over every voxel of its volume, from the oracle's per-record
    functions (record_stats and kin).  A trilinear sample is a blend of 8
    voxels, so the samples of a frame crowd towards the middle of the voxels'
    range; windows across the bare minimum and maximum would mostly show the
    empty tails."""
    key = (scene.kind, scene.size, scene.f16, scene.method)
    if key in _ranges:
        return _ranges[key]
    o, L = orc(), orc().lib()
    vol = volume(scene)
    fp = ctypes.POINTER(ctypes.c_float)
    nvox = DIMS[0] * DIMS[1] * DIMS[2]
    if scene.kind == "hist":
        nb = scene.size
        out = np.zeros(3, np.float32)
        pout = out.ctypes.data_as(fp)
        base = vol.ctypes.data
        vals = np.zeros((nvox, 4), np.float32)
        for v in range(nvox):
            rec = ctypes.cast(base + 4 * nb * v, fp)
            L.orc_record_stats(rec, nb, pout)
            vals[v, :3] = out
            vals[v, 3] = np.float32(L.orc_corner_mean(rec, nb)) * np.float32(50.0)  # K:479
        for m, k in ((1, 0), (2, 1), (3, 2), (7, 3)):
            _ranges[(scene.kind, nb, scene.f16, m)] = _p10_p90(vals[:, k])
    elif scene.kind == "codec":
        cb, t, e = vol
        c = o._codec(cb, t, e)
        out = np.zeros(3, np.float32)
        pout = out.ctypes.data_as(fp)
        vals = np.zeros((nvox, 3), np.float32)
        for v in range(nvox):
            L.orc_codec_stats(ctypes.byref(c), scene.size, v, pout)
            vals[v] = out
        for m in (4, 5, 6):
            _ranges[(scene.kind, scene.size, scene.f16, m)] = _p10_p90(vals[:, m - 4])
    else:
        wm, sg = vol
        K = scene.size
        bw, bs = wm.ctypes.data, sg.ctypes.data
        vals = np.zeros((nvox, 2), np.float32)
        for v in range(nvox):
            pw, ps = ctypes.cast(bw + 8 * K * v, fp), ctypes.cast(bs + 4 * K * v, fp)
            vals[v, 0] = L.orc_gmm_stat(pw, ps, K, 1)
            vals[v, 1] = L.orc_gmm_stat(pw, ps, K, 2)
        for m in (1, 2):
            _ranges[(scene.kind, K, scene.f16, m)] = _p10_p90(vals[:, m - 1])
    return _ranges[key]


def windows(lo, hi, n, tscale):
    """float32 transfer offsets of n windows across [lo, hi]: window i shows the
    statistic in [off_i, off_i + 1 / tscale], centred on the i-th of n equal
    parts of the range.  The same float32 values go to the GPU descriptor and to
    make_params."""
    centres = lo + (np.arange(n, dtype=np.float64) + 0.5) / n * (hi - lo)
    return (centres - 0.5 / tscale).astype(np.float32)


def scene_windows(scene):
    lo, hi = stat_range(scene)
    return windows(lo, hi, scene.nwin, scene.tscale)


def params(scene, toff):
    return orc().make_params(scene.W, scene.H, camera(scene.cam), density=scene.density,
                             transfer_offset=float(toff), transfer_scale=scene.tscale,
                             query_method=scene.method, m7_dims=scene.grid or DIMS)


def oracle_frame(scene, toff):
    """(rgba8 (H, W) uint32, rgba_f (H, W, 4) float32, samples (H, W) int32, -1 on
    a miss) of the oracle's current reading"""
    o, p, vol = orc(), params(scene, toff), volume(scene)
    if scene.kind == "hist":
        return o.render(vol, p)[:3]
    if scene.kind == "codec":
        return o.render_codec(*vol, p)[:3]
    r = o.render_gmm(vol[0], vol[1], DIMS, p)
    return r["out"], r["out_f"], r["out_n"]


# ---- the bar ----

def words_differ(a, b):
    """(H, W) bool: pixels with any float RGBA word different"""
    return np.any(np.ascontiguousarray(a).view(np.uint32) !=
                  np.ascontiguousarray(b).view(np.uint32), axis=-1)


def _ordered(f):
    """float32 words as integers in value order: adjacent floats differ by 1"""
    i = np.ascontiguousarray(f).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def assert_bit_parity(got, ref, what):
    """got, ref: (rgba8, rgba_f, samples).  RGBA8 equal, samples equal with misses
    reporting -1, float RGBA equal as uint32 words on every pixel."""
    g8, gf, gn = got
    r8, rf, rn = ref
    hit = rn >= 0
    assert np.array_equal(gn[hit], rn[hit]), f"{what}: samples per pixel differ"
    assert np.all(gn[~hit] == -1), f"{what}: miss pixels must report -1"
    assert np.array_equal(g8, r8), (
        f"{what}: {int(np.sum(g8 != r8))} RGBA8 pixels differ from the oracle")
    gw = np.ascontiguousarray(gf).view(np.uint32)
    rw = np.ascontiguousarray(rf).view(np.uint32)
    bad = gw != rw
    if bad.any():
        pix = np.argwhere(np.any(bad, axis=-1))
        y, x = (int(v) for v in pix[0])
        ulps = np.abs(_ordered(gf) - _ordered(rf))
        zero_sign = bool(np.all((gw[bad] | rw[bad]) == 0x80000000))
        raise AssertionError(
            f"{what}: float RGBA words of {len(pix)} pixels differ from the oracle; first "
            f"(x={x}, y={y}): got {gf[y, x].tolist()} oracle {rf[y, x].tolist()}, "
            f"{ulps[y, x].tolist()} ulps apart (max over the frame {int(ulps.max())}); "
            + ("every difference is only the sign of a zero" if zero_sign
               else "not only signs of zeros"))


# ---- the sensitivity of the scenes (tests/test_magnified_scenes.py) ----
# name -> 16 counts: pixels whose float RGBA words change over the scene's
# windows when corner j's statistic is nudged alone, [+1 ulp, corners 0..7],
# then [-1 ulp, corners 0..7].  Every count is >= MIN_LIT.
MIN_LIT = 4
PINNED = {
    "hist4-m1-C0": [16, 13, 15, 13, 16, 11, 10, 17, 16, 17, 12, 18, 15, 11, 11, 12],
    "hist4-m2-C0": [5, 8, 10, 11, 6, 9, 6, 5, 5, 8, 7, 10, 8, 8, 7, 8],
    "hist4-m3-C0": [12, 4, 9, 14, 8, 10, 11, 7, 6, 5, 12, 10, 15, 12, 11, 6],
    "hist4-m1-OBL": [18, 21, 18, 17, 14, 15, 11, 18, 10, 14, 16, 13, 9, 15, 23, 18],
    "hist4-m2-OBL": [7, 14, 5, 10, 15, 12, 12, 9, 11, 6, 10, 9, 8, 6, 6, 5],
    "hist4-m3-OBL": [11, 10, 9, 9, 11, 13, 10, 11, 6, 9, 8, 8, 9, 10, 12, 13],
    "hist8-m1-C0": [17, 18, 18, 14, 19, 14, 14, 11, 9, 12, 17, 21, 14, 15, 18, 22],
    "hist8-m2-C0": [12, 9, 11, 12, 13, 9, 15, 12, 5, 7, 9, 12, 8, 8, 16, 11],
    "hist8-m3-C0": [22, 22, 21, 24, 23, 21, 34, 37, 19, 19, 22, 20, 20, 21, 16, 15],
    "hist8-m1-OBL": [19, 24, 20, 20, 16, 16, 15, 11, 16, 7, 22, 21, 12, 21, 19, 15],
    "hist8-m2-OBL": [6, 9, 13, 13, 10, 11, 9, 10, 15, 17, 15, 9, 12, 12, 13, 10],
    "hist8-m3-OBL": [17, 27, 16, 18, 26, 22, 24, 21, 20, 15, 17, 13, 13, 16, 16, 16],
    "hist8-m1-SIDE": [17, 20, 14, 19, 18, 13, 20, 11, 22, 19, 24, 24, 18, 15, 20, 19],
    "hist8-m2-SIDE": [9, 11, 7, 13, 11, 13, 14, 9, 6, 7, 4, 9, 11, 12, 9, 10],
    "hist8-m3-SIDE": [18, 11, 14, 16, 17, 13, 25, 25, 21, 14, 22, 17, 23, 25, 25, 22],
    "hist1-m1-C0": [6, 7, 7, 6, 4, 10, 10, 6, 6, 6, 7, 7, 5, 4, 7, 5],
    "hist1-m2-C0": [9, 4, 10, 12, 7, 4, 12, 7, 12, 10, 8, 8, 8, 9, 10, 11],
    "hist1-m1-OBL": [10, 8, 7, 8, 9, 6, 9, 8, 11, 9, 10, 15, 8, 10, 10, 11],
    "hist1-m2-OBL": [5, 6, 8, 5, 5, 5, 4, 7, 10, 7, 8, 7, 8, 4, 12, 5],
    "hist2-m1-C0": [9, 10, 13, 13, 12, 9, 15, 16, 9, 11, 11, 10, 15, 14, 16, 14],
    "hist2-m2-C0": [16, 15, 11, 13, 14, 10, 14, 16, 13, 13, 11, 17, 19, 17, 15, 15],
    "hist2-m3-C0": [13, 9, 12, 6, 11, 6, 8, 6, 7, 5, 6, 4, 7, 8, 5, 5],
    "hist2-m1-OBL": [11, 9, 8, 7, 9, 9, 13, 12, 15, 9, 11, 16, 8, 9, 8, 17],
    "hist2-m2-OBL": [11, 12, 10, 10, 11, 15, 18, 16, 7, 8, 13, 16, 8, 9, 9, 9],
    "hist2-m3-OBL": [7, 6, 6, 9, 11, 8, 10, 8, 14, 11, 9, 16, 15, 8, 14, 6],
    "hist3-m1-C0": [5, 8, 11, 14, 15, 13, 10, 16, 9, 11, 16, 13, 7, 10, 9, 9],
    "hist3-m2-C0": [17, 13, 13, 9, 19, 12, 13, 8, 8, 7, 8, 10, 12, 14, 15, 13],
    "hist3-m3-C0": [5, 6, 6, 7, 6, 8, 6, 4, 12, 9, 13, 9, 4, 10, 7, 6],
    "hist5-m1-OBL": [9, 10, 7, 11, 16, 16, 7, 15, 18, 14, 15, 17, 18, 15, 9, 5],
    "hist5-m2-OBL": [16, 18, 15, 12, 12, 9, 17, 14, 15, 8, 14, 17, 4, 11, 11, 16],
    "hist5-m3-OBL": [23, 17, 12, 10, 12, 10, 9, 8, 17, 11, 15, 17, 15, 12, 13, 17],
    "hist16-m1-C0": [16, 9, 10, 7, 16, 12, 9, 4, 11, 11, 18, 15, 7, 12, 14, 17],
    "hist16-m2-C0": [7, 8, 4, 4, 9, 9, 10, 9, 8, 5, 9, 12, 10, 7, 12, 10],
    "hist16-m3-C0": [21, 20, 19, 13, 17, 10, 20, 17, 22, 15, 23, 20, 23, 20, 18, 12],
    "hist16-m1-OBL": [8, 11, 7, 10, 10, 10, 6, 4, 15, 13, 17, 14, 11, 14, 14, 16],
    "hist16-m2-OBL": [6, 7, 11, 9, 14, 7, 10, 8, 4, 7, 5, 6, 12, 7, 10, 8],
    "hist16-m3-OBL": [26, 22, 19, 9, 20, 15, 19, 21, 17, 13, 10, 13, 17, 18, 21, 27],
    "hist32-m1-C0": [15, 19, 11, 12, 14, 14, 11, 10, 6, 10, 10, 16, 7, 6, 10, 8],
    "hist32-m2-C0": [8, 8, 11, 13, 9, 8, 12, 12, 5, 11, 11, 9, 13, 13, 18, 11],
    "hist32-m3-C0": [18, 19, 13, 19, 14, 18, 19, 16, 24, 30, 20, 25, 23, 25, 10, 15],
    "hist32-m1-OBL": [9, 11, 8, 11, 12, 13, 10, 11, 11, 12, 16, 17, 10, 16, 15, 15],
    "hist32-m2-OBL": [8, 11, 9, 11, 16, 13, 18, 14, 10, 12, 5, 4, 9, 9, 8, 7],
    "hist32-m3-OBL": [17, 22, 21, 18, 21, 21, 20, 12, 13, 14, 21, 24, 21, 20, 18, 22],
    "hist8-m7-C0-g26x22x18": [12, 16, 19, 17, 17, 20, 18, 18, 14, 13, 10, 9, 19, 16, 19, 18],
    "hist8-m7-OBL-g26x22x18": [14, 8, 20, 12, 10, 17, 15, 15, 13, 13, 13, 11, 18, 9, 13, 12],
    "hist8-m7-SIDE-g26x22x18": [13, 17, 10, 9, 17, 8, 13, 14, 13, 15, 16, 12, 14, 10, 8, 17],
    "hist8-m7-OBL-g10x12x20": [14, 15, 12, 15, 24, 17, 18, 18, 16, 15, 14, 7, 19, 17, 17, 15],
    "codec8-m4-C0": [15, 12, 13, 10, 16, 16, 14, 8, 12, 6, 7, 7, 13, 13, 11, 12],
    "codec8-m5-C0": [10, 9, 6, 10, 9, 11, 10, 7, 8, 6, 7, 12, 10, 5, 12, 13],
    "codec8-m6-C0": [11, 13, 10, 11, 7, 8, 15, 12, 9, 10, 8, 9, 12, 12, 14, 16],
    "codec8-m4-OBL": [8, 7, 6, 6, 8, 8, 12, 13, 8, 13, 13, 16, 6, 6, 14, 13],
    "codec8-m5-OBL": [7, 7, 12, 14, 8, 13, 10, 11, 5, 11, 7, 11, 7, 7, 6, 8],
    "codec8-m6-OBL": [11, 8, 9, 9, 4, 6, 9, 6, 11, 10, 9, 6, 9, 14, 9, 10],
    "codec32-m4-OBL": [8, 12, 7, 8, 12, 11, 9, 10, 18, 14, 9, 9, 13, 16, 9, 7],
    "codec32-m5-OBL": [12, 8, 4, 5, 4, 4, 4, 10, 6, 5, 7, 6, 9, 10, 4, 9],
    "codec32-m6-OBL": [13, 17, 13, 19, 15, 13, 17, 13, 8, 6, 10, 13, 7, 9, 5, 8],
    "gmm8-m1-OBL": [7, 6, 5, 8, 8, 8, 7, 8, 8, 9, 8, 8, 12, 11, 16, 9],
    "gmm8h-m1-C0": [17, 18, 12, 12, 14, 18, 12, 16, 9, 14, 11, 8, 8, 8, 10, 12],
    "gmm8-m2-OBL": [6, 7, 13, 12, 8, 9, 9, 15, 8, 6, 15, 4, 10, 10, 12, 8],
    "gmm8h-m2-C0": [5, 7, 10, 11, 5, 5, 8, 8, 8, 7, 6, 6, 11, 5, 5, 7],
    "gmm16-m1-OBL": [14, 13, 9, 9, 12, 11, 14, 13, 16, 17, 16, 8, 14, 18, 11, 9],
    "gmm16h-m1-C0": [11, 14, 9, 11, 9, 11, 12, 10, 10, 7, 10, 13, 15, 16, 21, 19],
    "gmm16-m2-OBL": [15, 12, 12, 15, 8, 8, 9, 9, 8, 14, 9, 10, 5, 9, 9, 13],
    "gmm16h-m2-C0": [11, 10, 8, 16, 5, 9, 7, 12, 6, 9, 9, 14, 13, 12, 16, 11],
    "gmm32-m1-OBL": [12, 14, 17, 13, 14, 11, 16, 16, 11, 15, 17, 14, 12, 17, 10, 13],
    "gmm32h-m1-C0": [4, 4, 11, 15, 7, 7, 10, 12, 11, 11, 6, 8, 6, 12, 5, 7],
    "gmm32-m2-OBL": [5, 9, 7, 9, 11, 6, 11, 10, 13, 10, 9, 8, 10, 12, 8, 9],
    "gmm32h-m2-C0": [7, 9, 9, 5, 12, 13, 9, 12, 6, 8, 10, 14, 5, 7, 9, 9],
    "hist1h-m1-OBL": [6, 8, 12, 6, 7, 4, 11, 6, 9, 6, 7, 10, 12, 8, 5, 8],
    "hist1h-m2-OBL": [8, 4, 9, 14, 10, 4, 6, 10, 20, 11, 11, 7, 4, 9, 7, 7],
    "hist8h-m1-OBL": [13, 9, 12, 13, 14, 22, 17, 25, 17, 17, 15, 15, 11, 11, 14, 18],
    "hist8h-m2-OBL": [7, 11, 7, 14, 11, 16, 7, 13, 18, 14, 16, 16, 12, 10, 16, 12],
    "hist8h-m3-OBL": [16, 18, 14, 21, 16, 19, 16, 20, 22, 26, 18, 19, 25, 25, 22, 21],
    "hist32h-m1-OBL": [9, 9, 10, 11, 9, 12, 12, 7, 12, 11, 11, 9, 16, 17, 13, 11],
    "hist32h-m2-OBL": [7, 12, 11, 10, 8, 12, 12, 8, 9, 12, 6, 9, 6, 10, 9, 8],
    "hist32h-m3-OBL": [22, 21, 22, 15, 18, 21, 20, 14, 20, 19, 16, 20, 19, 17, 15, 19],
}
