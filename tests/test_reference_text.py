"""The oracle against the reference's own kernel text, compiled for the CPU.

oracle/vr_oracle.c restates d_basicDataProcessing and d_render under the rules in
its header: ISO C semantics as written, promotions as the source implies, left to
right, no fused multiply-add.  oracle/ref/build_ref.py compiles the text of those
two kernels as host C++ with -ffp-contract=off against shim headers, so the
compiled text is that claim's definition and every comparison here is word for
word: there is no tolerance to choose.

What this pins: every C++ semantic of the two kernels (promotions, association,
branch and exit order, the refresh logic of method 7, the codec decode).  What it
cannot pin: the shim's texture fetch, rsqrtf and log(float) are our reading of
CUDA (oracle/ref/shim/helper_cuda.h), the same reading the oracle takes.

CPU only.  The module skips only where there is neither a reference directory
nor a built library (a checkout on a machine that never saw the reference).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as graft  # noqa: E402
import magnify  # noqa: E402

R = graft.load_reference()

if not R.have_reference_dir() and not any(R.available(n) for n in R.recipe.VARIANTS):
    pytest.skip("no reference directory and no oracle/_ref library: nothing to compare with",
                allow_module_level=True)

NX, NY, NZ = R.DIMS
NVOX = R.NVOX
W, H = 64, 48
PREFILL = 0x5AA5C33C  # what a miss must leave in the frame (K:302-303)
M7_OTHER = (20, 30, 7)  # a method-7 grid that is not the volume's


@pytest.fixture(scope="module")
def orc():
    o = graft.load_oracle()
    o.set_reading()
    yield o
    o.set_reading()


def ref_lib(name):
    """a missing library is a failure: build() makes all of them wherever the
    reference directory exists"""
    assert R.available(name), (
        f"oracle/_ref/libref_{name}.so is missing: run __graft_entry__.build() with the "
        "reference directory in place")
    lib = R.load(name)
    lib.set_weight_trunc(False)
    return lib


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- cameras ----

def cameras():
    magnify.camera("C0")  # loads the package's camera module without the package
    cam = magnify._camera_mod
    # an exact quarter turn about y, eye at (4, 0, 0): the matrix holds only 0 and
    # +-1, so the frame's middle column and row give rays with an exactly zero
    # direction component (two for the centre pixel) and intersectBox divides by
    # zero (K:140); QUARTER_EDGE moves the eye onto the plane y = 1, where
    # inf * (boxmax - o) is NaN and fminf / fmaxf must drop it (K:141-146)
    quarter = np.array([0, 0, 1, 4, 0, 1, 0, 0, -1, 0, 0, 0], np.float32)
    edge = quarter.copy()
    edge[7] = 1.0
    return {
        "C0": cam.single_test_inv_view(),
        "OBL": cam.display_inv_view((30.0, 45.0)),
        "INSIDE": cam.display_inv_view((20.0, -35.0), (0.0, 0.0, -0.6)),  # eye in the box
        "QUARTER": quarter,
        "QUARTER_EDGE": edge,
    }


# the three sets of test_render_parameters (tests/test_gpu_parity.py) after the default
PARAM_SETS = [
    dict(density=0.05, brightness=1.0, transfer_offset=0.0, transfer_scale=1.0),
    dict(density=0.2, brightness=1.5, transfer_offset=0.1, transfer_scale=1.3),
    dict(density=1.0, brightness=0.7, transfer_offset=-0.2, transfer_scale=0.5),
    dict(density=0.01, brightness=2.0, transfer_offset=0.05, transfer_scale=2.0),
]
NWIN = 4  # narrow windows across the statistic's 10th-90th percentile


def window_sets(values):
    lo, hi = magnify._p10_p90(np.asarray(values, np.float32))
    return [dict(density=0.5, brightness=1.0, transfer_offset=float(t), transfer_scale=256.0)
            for t in magnify.windows(lo, hi, NWIN, 256.0)]


# ---- volumes (computed once, read-only) ----

def spiky(nb, seed):
    """magnify._random_hist's records at the reference's shape: spiky, a tenth of
    the bins exactly 0"""
    rng = np.random.default_rng(seed)
    p = rng.random((NZ, NY, NX, nb))
    p = p * p * p
    p[rng.random(p.shape) < 0.1] = 0.0
    p[..., 0] += 1e-3
    p /= magnify._total(p)
    return np.ascontiguousarray(p.astype(np.float32))


def hand_made(nb):
    sub = np.float32(1e-41)  # subnormal
    recs = []
    for k in (0, nb // 2, nb - 1):
        r = np.zeros(nb, np.float32)
        r[k] = 1.0
        recs.append(r)                                   # one bin equal to 1
    recs.append(np.full(nb, 1.0 / nb, np.float32))       # uniform
    recs.append(np.zeros(nb, np.float32))                # all zero
    recs.append(np.full(nb, 2.0 / nb, np.float32))       # sums to 2
    r = np.zeros(nb, np.float32)
    r[1], r[2] = 1.0, sub
    recs.append(r)                                       # a subnormal beside a 1
    r = np.full(nb, sub, np.float32)
    r[nb - 1] = 1.0
    recs.append(r)
    r = np.full(nb, 1.0 / nb, np.float32)
    r[0], r[3] = -0.25, 0.25 + 2.0 / nb
    recs.append(r)                                       # a negative bin (the <= 0 branch)
    recs.append(np.full(nb, -1.0 / nb, np.float32))
    return recs


_cache = {}


def hist_volume(nb, family):
    key = (nb, family)
    if key not in _cache:
        if family == "spiky":
            v = spiky(nb, 1000 + nb)
        elif family == "synth":
            v = graft.load_oracle().synth_volume(NX, NY, NZ, nb)
        else:  # the hand-made records first, spiky records behind them
            v = spiky(nb, 3000 + nb)
            flat = v.reshape(NVOX, nb)
            for i, r in enumerate(hand_made(nb)):
                flat[i] = r
        v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def codec_volume(nb):
    """synth_codec at the reference's shape, with the decode's edges written into
    its first voxels.  Error bin ids stay inside [0, nb): the reference writes out
    of bounds for id == nb (K:810 admits it, K:817 stores), which the oracle
    skips by choice (vr_oracle.c, orc_codec_decode), so such inputs have no
    defined reference result and are kept out."""
    key = (nb, "codec")
    if key in _cache:
        return _cache[key]
    cb, tp, er = graft.load_oracle().synth_codec(NX, NY, NZ, nb)
    tp = np.concatenate([tp, np.zeros((1, nb), np.float32)])  # an all-zero template
    zero_t = tp.shape[0] - 1
    slots = er.shape[-2]
    assert slots == nb
    cbf, erf = cb.reshape(NVOX, 4), er.reshape(NVOX, slots, 2)
    v = 0
    for flip in (0, 1):
        for shift in (0, nb - 1):
            for ne in (0, slots):  # NE 0 and every slot used
                cbf[v] = (v % zero_t, shift, flip, ne)
                erf[v, :, 0] = np.arange(slots) % nb
                erf[v, :, 1] = np.where(np.arange(slots) % 2, 0.01, -0.004)
                v += 1
    # an error that drives a bin negative: the clamp of K:818
    cbf[v] = (1, 3, 1, 2)
    erf[v, 0] = (2, -0.9)
    erf[v, 1] = (2, 0.05)   # added to the clamped 0, not to the negative value
    v += 1
    # a record whose total is 0 (K:833): the zero template, and one cancelled to 0
    cbf[v] = (zero_t, 0, 0, 0)
    v += 1
    cbf[v] = (zero_t, 2, 1, 1)
    erf[v, 0] = (nb - 1, -0.5)
    v += 1
    assert erf[..., 0].min() >= 0 and erf[..., 0].max() < nb
    for a in (cb, tp, er):
        a.setflags(write=False)
    _cache[key] = (cb, tp, er)
    return _cache[key]


def oracle_stats(orc, vol, nb):
    """(record_stats (NVOX, 3), corner_mean (NVOX,)) through the oracle's C entry points"""
    L = orc.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    out = np.zeros(3, np.float32)
    pout = out.ctypes.data_as(fp)
    base = vol.ctypes.data
    stats = np.zeros((NVOX, 3), np.float32)
    cm = np.zeros(NVOX, np.float32)
    for v in range(NVOX):
        rec = ctypes.cast(base + 4 * nb * v, fp)
        L.orc_record_stats(rec, nb, pout)
        stats[v] = out
        cm[v] = L.orc_corner_mean(rec, nb)
    return stats, cm


def oracle_codec_stats(orc, codec, nb):
    L = orc.lib()
    c = orc._codec(*codec)
    out = np.zeros(3, np.float32)
    pout = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    stats = np.zeros((NVOX, 3), np.float32)
    for v in range(NVOX):
        L.orc_codec_stats(ctypes.byref(c), nb, v, pout)
        stats[v] = out
    return stats


# ---- record statistics ----

@pytest.mark.parametrize("family", ["spiky", "synth", "hand"])
@pytest.mark.parametrize("nb", [32, 8])
def test_record_statistics(orc, nb, family):
    """originalHistogramData (K:736-773) over 25 000 records against
    orc_record_stats, all 75 000 words.  The corner mean of method 7 (K:355-366)
    is the same expression as the mean of K:742-747 before its division, so
    orc_corner_mean / 0.0217 must give the reference's .x word too; the method-7
    frames below check the corner mean undivided."""
    ref = ref_lib(f"b{nb}")
    vol = hist_volume(nb, family)
    ref.init(vol)
    plane, _ = ref.basic_data_processing()
    stats, cm = oracle_stats(orc, vol, nb)
    bad = words(stats) != words(plane[:, :3])
    print(f"{nb} bins {family}: {int(bad.sum())} of {bad.size} statistic words differ")
    assert not bad.any(), (f"{int(bad.sum())} words differ; first voxel "
                           f"{int(np.argwhere(bad.any(axis=1))[0, 0])}")
    via_cm = (cm.astype(np.float64) / 0.0217).astype(np.float32)  # K:758
    assert np.array_equal(words(via_cm), words(plane[:, 0]))
    if family == "synth":
        assert np.any((vol > 0) & (vol < np.finfo(np.float32).tiny)), "no subnormal bins"
    if family == "hand":
        assert np.isfinite(plane[:len(hand_made(nb)), :3]).all()


@pytest.mark.parametrize("nb", [32, 8])
def test_codec_statistics(orc, nb):
    """fractalHistogramData (K:775-871) against orc_codec_stats: both flips, shifts
    0 and nb - 1, NE 0 and every slot, the clamp of K:818, totals of 0 (K:833)"""
    ref = ref_lib(f"b{nb}")
    codec = codec_volume(nb)
    ref.init(hist_volume(nb, "spiky"), codec)
    _, plane = ref.basic_data_processing()
    stats = oracle_codec_stats(orc, codec, nb)
    bad = words(stats) != words(plane[:, :3])
    print(f"{nb} bins codec: {int(bad.sum())} of {bad.size} statistic words differ")
    assert not bad.any(), (f"{int(bad.sum())} words differ; first voxel "
                           f"{int(np.argwhere(bad.any(axis=1))[0, 0])}")
    assert np.all(plane[9:11, :3] == 0.0)  # the two records whose total is 0


# ---- frames ----

def oracle_frame(orc, kind, data, p):
    """(RGBA8 with the prefill where the ray misses, saturated float RGBA, samples)"""
    if kind == "hist":
        r8, rf, rn, _ = orc.render(data, p)
    elif kind == "codec":
        r8, rf, rn, _ = orc.render_codec(*data, p)
    else:
        r8, rf, rn, _ = orc.render_flex(data, p)
    return np.where(rn >= 0, r8, np.uint32(PREFILL)), rf, rn


def frame_cases(orc, nb, ref):
    """(method, method-7 grid, kind, data, parameter sets) for methods 1-7; binds the
    volumes to ref and runs its basicDataProcessing"""
    vol = hist_volume(nb, "spiky")
    codec = codec_volume(nb)
    ref.init(vol, codec)
    plane, cplane = ref.basic_data_processing()
    _, cm = oracle_stats(orc, vol, nb)
    cases = []
    for method, grid in ((1, R.DIMS), (2, R.DIMS), (3, R.DIMS), (7, R.DIMS), (7, M7_OTHER)):
        vals = plane[:, method - 1] if method < 7 else cm * np.float32(50.0)
        cases.append((method, grid, "hist", vol, PARAM_SETS + window_sets(vals)))
    for method in (4, 5, 6):
        cases.append((method, R.DIMS, "codec", codec,
                      PARAM_SETS + window_sets(cplane[:, method - 4])))
    return cases


def compare_frames(orc, ref, cases, cams):
    """renders every case on every camera with both; returns (frames, differing
    frames, differing pixels, hit pixels, miss pixels, the first difference).  A
    pixel differs if its RGBA8 word differs, if one side hits where the other
    misses, or if any word of the saturated float RGBA that is packed differs
    (the reference never stores it; the shim's __saturatef keeps it)."""
    frames = bad_frames = bad_pix = hits = misses = 0
    first = None
    for method, grid, kind, data, sets in cases:
        for cname, m in cams.items():
            for kw in sets:
                p = orc.make_params(W, H, m, query_method=method, m7_dims=grid, **kw)
                got, got_f = ref.render(p, prefill=PREFILL, want_float=True)
                want, want_f, rn = oracle_frame(orc, kind, data, p)
                hit = rn >= 0
                written = ~np.isnan(got_f).any(axis=-1)
                fbad = np.zeros((H, W), bool)
                both = hit & written
                fbad[both] = np.any(words(got_f[both]) != words(want_f[both]), axis=-1)
                n = int(np.sum((got != want) | (hit != written) | fbad))
                frames += 1
                hits += int(np.sum(rn >= 0))
                misses += int(np.sum(rn < 0))
                if n:
                    bad_frames += 1
                    bad_pix += n
                    first = first or f"method {method} grid {grid} {cname} {kw}: {n} pixels"
    return frames, bad_frames, bad_pix, hits, misses, first


@pytest.mark.parametrize("nb", [32, 8])
def test_frames(orc, nb):
    """d_render's RGBA8, and the float RGBA it packs, against the oracle's: methods 1/2/3/7 (method-7 grid equal
    to the volume's and not) and 4/5/6, five cameras, four parameter sets and four
    narrow windows each, misses included through the prefill"""
    ref = ref_lib(f"b{nb}")
    cases = frame_cases(orc, nb, ref)
    frames, bad_frames, bad_pix, hits, misses, first = compare_frames(orc, ref, cases, cameras())
    print(f"{nb} bins: {frames} frames, {hits} hit and {misses} miss pixels, "
          f"{bad_frames} frames / {bad_pix} pixels differ")
    assert misses > 0 and hits > 0
    assert bad_frames == 0, f"{bad_frames} of {frames} frames differ; first: {first}"


def test_flex_frames(orc):
    """methods 8/9/0 (K:654-680): the render half only, on a block table from the
    oracle's own prepass presented as the 500^3 flexBlockTex; the reference's
    prepass kernels sum floats with atomics in no defined order and are out of
    scope"""
    ref = ref_lib("b32")
    ref.init(hist_volume(32, "spiky"))
    t = orc.synth_flex(20, 6, 32, ntemplates=8, seed=9)
    blocks = orc.flex_process(t)  # (4, 4, 4, 4)
    ref.bind_flex(blocks)
    comp = {8: 2, 9: 0, 0: 1}
    cases = [(method, (1, 1, 1), "flex", blocks,
              PARAM_SETS + window_sets(blocks[..., comp[method]].reshape(-1)))
             for method in (8, 9, 0)]
    frames, bad_frames, bad_pix, hits, misses, first = compare_frames(orc, ref, cases, cameras())
    print(f"flex: {frames} frames, {hits} hit pixels, {bad_frames} frames / {bad_pix} pixels differ")
    assert bad_frames == 0, f"{bad_frames} of {frames} frames differ; first: {first}"


# ---- the canary: the comparison can fail ----

def _canary_cases(orc, ref):
    return [c for c in frame_cases(orc, 32, ref) if c[0] in (1, 3, 5)]


def test_canary_truncated_weights(orc):
    """texture filter weights truncated instead of rounded (a shim switch): the
    frame comparison must fail"""
    ref = ref_lib("b32")
    cases = _canary_cases(orc, ref)
    cams = {k: v for k, v in cameras().items() if k in ("C0", "OBL")}
    ref.set_weight_trunc(True)
    try:
        _, bad_frames, bad_pix, _, _, _ = compare_frames(orc, ref, cases, cams)
    finally:
        ref.set_weight_trunc(False)
    print(f"canary, truncated weights: {bad_frames} frames / {bad_pix} pixels differ")
    assert bad_frames > 0
    assert compare_frames(orc, ref, cases, cams)[1] == 0  # and the switch is off again


def test_canary_far_exit(orc):
    """the far exit of K:703 taken one step early (the b32_exit_canary build: `t +
    tstep > tfar`): the frame comparison must fail.  Swapping the far exit with the
    opacity exit of K:698 alone cannot change a pixel, since both leave the loop
    after the same composite; what a misread exit order changes is how many
    samples a ray takes, and this canary takes one fewer."""
    ref = ref_lib("b32_exit_canary")
    cases = _canary_cases(orc, ref)
    cams = {k: v for k, v in cameras().items() if k in ("C0", "OBL")}
    _, bad_frames, bad_pix, _, _, _ = compare_frames(orc, ref, cases, cams)
    print(f"canary, far exit one step early: {bad_frames} frames / {bad_pix} pixels differ")
    assert bad_frames > 0


# ---- what an RGBA8 frame can resolve (a measurement, not a bar) ----

def test_rgba8_resolution_of_the_windows(orc):
    """The reference writes RGBA8 only.  How much of a last-bit error in one
    corner's statistic does an RGBA8 frame show, and how much the float RGBA the
    shim keeps?  The oracle's statistic nudge moves one corner by +-1 ulp; the
    figures are the pixels whose RGBA8 word, and whose float RGBA words, change,
    per narrow window of the oblique view and nudge.  Printed and recorded in
    DESIGN.md section 3; the statistics themselves are held to the last bit by
    the plane comparisons above, the frames are there for the march."""
    cases = [c for c in frame_cases(orc, 32, ref_lib("b32"))
             if c[0] in (1, 2, 3) or c[:2] == (7, R.DIMS)]
    m = cameras()["OBL"]
    total_hit = 0
    figures = {}
    try:
        for method, grid, kind, data, sets in cases:
            changed, changed_f = [], []
            for kw in sets[len(PARAM_SETS):]:
                p = orc.make_params(W, H, m, query_method=method, m7_dims=grid, **kw)
                orc.set_stat_nudge()
                base, base_f, rn = oracle_frame(orc, kind, data, p)
                total_hit = int(np.sum(rn >= 0))
                for corner in (0, 7):
                    for ulps in (1, -1):
                        orc.set_stat_nudge(ulps, 1 << corner)
                        f8, ff, _ = oracle_frame(orc, kind, data, p)
                        changed.append(int(np.sum(f8 != base)))
                        changed_f.append(int(np.sum(np.any(words(ff) != words(base_f), axis=-1))))
            figures[method] = (changed, changed_f)
    finally:
        orc.set_stat_nudge()
    for method, (changed, changed_f) in figures.items():
        print(f"method {method}: RGBA8 pixels changed by a 1-ulp nudge of one corner, per window "
              f"and nudge: {changed} (of {total_hit} hit pixels); mean "
              f"{sum(changed) / len(changed):.2f}; pixels with a float RGBA word changed: "
              f"{changed_f}, mean {sum(changed_f) / len(changed_f):.2f}")
