"""The sensitivity of the decode-magnifying scenes, proven on the CPU.

tests/test_gpu_bitparity.py compares the GPU marches with the oracle word for
word on the scenes of tests/magnify.py.  That says something only if a decode
that is wrong in its last bit changes those frames.  Here the oracle itself
plays that decode: every scene is rendered canonically and again with the
statistic of each of the 8 corners of a sample nudged alone by +1 and by -1 ulp
(oracle set_stat_nudge), and the pixels whose float RGBA words change are
counted over the scene's windows.

- the counts are pinned (magnify.PINNED), so a change of the oracle, of a scene
  or of the windows cannot silently change what the scenes see;
- every corner and either sign changes at least magnify.MIN_LIT pixels;
- magnify.assert_bit_parity fails on every nudged frame that differs, and on
  every scene; the share of them the 1e-4 bar of test_gpu_parity.assert_parity
  would have passed is recorded, nothing asserted on it.

`python tests/test_magnified_scenes.py` prints the table to pin and the shares.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import magnify as M  # noqa: E402
from test_gpu_parity import assert_parity  # noqa: E402  (the present bar, for the record)

_measured = {}


def _fails(check, got, ref):
    try:
        check(got, ref, "nudged")
    except AssertionError:
        return True
    return False


def measure(scene):
    """(16 counts as magnify.PINNED holds them, nudged frames the 1e-4 bar passes,
    nudged frames the bit bar passes, nudged frames, windows on which the frame
    with corner 0 off by +1 ulp fails the bit bar)"""
    if scene.name in _measured:
        return _measured[scene.name]
    o = M.orc()
    counts = [0] * 16
    old_pass = bit_pass = frames = c0_fail = 0
    try:
        for toff in M.scene_windows(scene):
            o.set_reading()
            ref = M.oracle_frame(scene, toff)
            k = 0
            for ulps in (1, -1):
                for corner in range(8):
                    o.set_stat_nudge(ulps, 1 << corner)
                    got = M.oracle_frame(scene, toff)
                    n = int(np.sum(M.words_differ(got[1], ref[1])))
                    counts[k] += n
                    k += 1
                    frames += 1
                    old_pass += not _fails(assert_parity, got, ref)
                    same = n == 0 and np.array_equal(got[2], ref[2])
                    assert _fails(M.assert_bit_parity, got, ref) == (not same), (
                        f"{scene.name}: assert_bit_parity and the word count disagree")
                    bit_pass += same
                    c0_fail += (ulps, corner) == (1, 0) and not same
    finally:
        o.set_reading()
    _measured[scene.name] = (counts, old_pass, bit_pass, frames, c0_fail)
    return _measured[scene.name]


@pytest.mark.parametrize("name", [s.name for s in M.SCENES])
def test_scene_sees_a_last_bit_error(name):
    scene = M.BY_NAME[name]
    counts, old_pass, bit_pass, frames, c0_fail = measure(scene)
    print(f"{name}: pixels changed per corner, +1 ulp {counts[:8]}, -1 ulp {counts[8:]}; "
          f"the 1e-4 bar passes {old_pass} of {frames} nudged frames, the bit bar {bit_pass}")
    assert min(counts) >= M.MIN_LIT, f"{name}: a corner or a sign changes too few pixels: {counts}"
    assert counts == M.PINNED[name], f"{name}: measured {counts}"
    # the deliberate check: an oracle frame with one corner off by +1 ulp, given to
    # assert_bit_parity as "got", fails on this scene (measure() feeds it every
    # nudged frame and holds its verdict against the word count)
    assert c0_fail >= 1, f"{name}: no window shows corner 0 off by +1 ulp"


def test_pinned_table():
    assert sorted(M.PINNED) == sorted(s.name for s in M.SCENES)
    for name, counts in M.PINNED.items():
        assert len(counts) == 16 and min(counts) >= M.MIN_LIT, (name, counts)
    for s in M.SCENES:
        assert 1 <= s.nwin <= 8, s


def test_scene_table_covers_the_families():
    """what tests/test_gpu_bitparity.py draws on"""
    for nb in (4, 8):
        assert {s.cam for s in M.select("hist", [nb], [1, 2, 3])} >= {"C0", "OBL"}
    assert "SIDE" in {s.cam for s in M.select("hist", [8])}
    for nb in (1, 2, 3, 5, 16, 32):
        want = {1, 2, 3} if nb > 1 else {1, 2}
        assert {s.method for s in M.select("hist", [nb])} == want
    assert not M.select("hist", [1], [3]), "the entropy of one bin is constant"
    assert {s.grid for s in M.select("hist", [8], [7])} == {M.DIMS, M.M7_GRID}
    assert {(s.size, s.method) for s in M.select("codec")} == {
        (b, m) for b in (8, 32) for m in (4, 5, 6)}
    for f16 in (False, True):
        assert {(s.size, s.method) for s in M.select("gmm", f16=f16)} == {
            (K, m) for K in (8, 16, 32) for m in (1, 2)}
    assert {s.size for s in M.select("hist", f16=True)} >= {1, 8, 32}


def test_windows():
    w = M.windows(0.25, 0.75, 4, 256.0)
    assert w.dtype == np.float32 and w.shape == (4,)
    centres = w.astype(np.float64) + 0.5 / 256.0
    assert np.allclose(centres, [0.3125, 0.4375, 0.5625, 0.6875], rtol=0, atol=1e-7)
    for s in (M.BY_NAME["hist1-m2-C0"], M.BY_NAME["codec8-m5-OBL"], M.BY_NAME["gmm8-m2-OBL"]):
        lo, hi = M.stat_range(s)
        offs = M.scene_windows(s)
        assert len(offs) == s.nwin and lo < offs[0] + 0.5 / s.tscale < offs[-1] + 1 / s.tscale < hi
        # the descriptor's float and make_params' float are the same float32
        assert M.params(s, offs[1]).transfer_offset == offs[1]


def test_nudge_off_is_the_canonical_reading():
    """nudge (0, any mask) and (any ulps, 0) render the canonical frame; a nudged
    render differs; set_reading() clears the nudge"""
    o = M.orc()
    for name in ("hist8-m2-OBL", "hist8-m7-OBL-g10x12x20", "codec8-m4-C0", "gmm8-m1-OBL"):
        s = M.BY_NAME[name]
        toff = M.scene_windows(s)[s.nwin // 2]
        o.set_reading()
        ref = M.oracle_frame(s, toff)
        try:
            for ulps, mask in ((0, 0xFF), (3, 0)):
                o.set_stat_nudge(ulps, mask)
                got = M.oracle_frame(s, toff)
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                           for a, b in zip(got, ref)), (name, ulps, mask)
            o.set_stat_nudge(1, 0xFF)
            assert np.any(M.words_differ(M.oracle_frame(s, toff)[1], ref[1])), name
            o.set_reading()
            M.assert_bit_parity(M.oracle_frame(s, toff), ref, name)
        finally:
            o.set_reading()


def _frame():
    f = np.zeros((3, 4, 4), np.float32)
    f[1, 2] = (0.25, 0.5, 0.0, 1.0)
    n = np.full((3, 4), 7, np.int32)
    n[0, 0] = -1
    return np.zeros((3, 4), np.uint32), f, n


def test_assert_bit_parity_reports():
    ref = _frame()
    M.assert_bit_parity(_frame(), ref, "same")
    got = _frame()
    got[1][1, 2, 1] = np.nextafter(np.float32(0.5), np.float32(1.0))
    got[1][2, 3, 0] = np.float32(-0.0)
    with pytest.raises(AssertionError) as e:
        M.assert_bit_parity(got, ref, "one ulp")
    msg = str(e.value)
    assert "2 pixels differ" in msg and "(x=2, y=1)" in msg and "[0, 1, 0, 0] ulps" in msg
    assert "not only signs of zeros" in msg
    got = _frame()
    got[1][2, 3, 0] = np.float32(-0.0)
    with pytest.raises(AssertionError, match="1 pixels differ.*only the sign of a zero"):
        M.assert_bit_parity(got, ref, "minus zero")
    got = _frame()
    got[2][0, 0] = -2  # a miss must report -1
    with pytest.raises(AssertionError, match="miss pixels"):
        M.assert_bit_parity(got, ref, "miss")
    got = _frame()
    got[2][1, 1] = 8
    with pytest.raises(AssertionError, match="samples per pixel"):
        M.assert_bit_parity(got, ref, "samples")
    got = _frame()
    got[0][1, 1] = 1
    with pytest.raises(AssertionError, match="RGBA8"):
        M.assert_bit_parity(got, ref, "rgba8")


if __name__ == "__main__":
    total = [0, 0, 0]
    rows = []
    print("PINNED = {")
    for s in M.SCENES:
        counts, old_pass, bit_pass, frames, _ = measure(s)
        print(f'    "{s.name}": {counts},')
        rows.append((s, counts, old_pass, bit_pass, frames))
    print("}")
    for s, counts, old_pass, bit_pass, frames in rows:
        print(f"| {s.name} | {s.W}x{s.H} | {s.tscale:g} | {s.nwin} | {min(counts)} .. "
              f"{max(counts)} | {old_pass} of {frames} | {bit_pass} of {frames} |")
        total[0] += old_pass
        total[1] += bit_pass
        total[2] += frames
    print("total: the 1e-4 bar passes %d, the bit bar %d of %d nudged frames" % tuple(total))
    # for comparison: the same nudges on plain frames,
    # transfer_scale 1, offset 0, density 0.05
    o = M.orc()
    plain = [0, 0, 0]
    for name in ("hist8-m1-OBL", "hist8-m2-OBL", "hist8-m3-OBL", "hist32-m3-C0",
                 "hist8-m7-OBL-g26x22x18", "codec8-m4-C0", "gmm16-m1-OBL", "gmm16-m2-OBL"):
        s = M.BY_NAME[name]._replace(tscale=1.0, density=0.05)
        o.set_reading()
        ref = M.oracle_frame(s, 0.0)
        counts = []
        for ulps in (1, -1):
            for corner in range(8):
                o.set_stat_nudge(ulps, 1 << corner)
                got = M.oracle_frame(s, 0.0)
                counts.append(int(np.sum(M.words_differ(got[1], ref[1]))))
                plain[0] += not _fails(assert_parity, got, ref)
                plain[1] += not _fails(M.assert_bit_parity, got, ref)
                plain[2] += 1
        o.set_reading()
        print(f"plain {name}: pixels changed {counts}")
    print("plain: the 1e-4 bar passes %d, the bit bar %d of %d nudged frames" % tuple(plain))
