"""Code-object checks of the lit plane march in the built libvr.so (CPU: reads the
gfx950 kernel metadata notes, runs nothing).  Exactly the four k_march_lit<GM, CROSS>
instances ship -- GM 1 or 2 (32-bit and 64-bit plane indices), CROSS false or true;
none uses scratch (private segment 0, no dynamic stack, at most 128 VGPRs: two of
its four waves per SIMD at the least), each holds the table's 4 KiB of LDS and nothing
else, and each takes the arguments of k_march_plane_tf and the 16 bytes of the light,
so Params has not grown."""
import re

from test_crossing_codeobj import _notes

LIT = re.compile(r"^_ZN2vr11k_march_litILi(\d+)ELb([01])EEE")
TF = re.compile(r"^_ZN2vr16k_march_plane_tfILi(\d+)ELb([01])EEE")
WANT = {(gm, cross) for gm in (1, 2) for cross in (0, 1)}


def _instances(pattern):
    return {tuple(int(v) for v in m.groups()): meta for n, meta in _notes().items()
            for m in [pattern.match(n or "")] if m}


def test_exactly_the_four_instances_ship():
    lit = _instances(LIT)
    assert set(lit) == WANT, sorted(WANT ^ set(lit))
    assert len([n for n in _notes() if n and "k_march_lit" in n]) == 4


def test_no_scratch_and_the_table_s_lds():
    lit = _instances(LIT)
    assert len(lit) == 4, sorted(lit)
    bad = {k: v for k, v in lit.items()
           if v["private_segment_fixed_size"] or v["dynamic_stack"]
           or v["group_segment_fixed_size"] != 4096}
    assert not bad, bad
    assert all(0 < v["vgpr_count"] <= 128 for v in lit.values()), \
        {k: v["vgpr_count"] for k, v in lit.items()}


def test_the_march_takes_the_arguments_of_k_march_plane_tf_and_the_light():
    lit, tf = _instances(LIT), _instances(TF)
    assert set(tf) == WANT, sorted(tf)
    for key in sorted(WANT):
        assert lit[key]["kernarg_segment_size"] == tf[key]["kernarg_segment_size"] + 16 > 16, key
