"""Code-object checks of the two-plane transfer-function march in the built libvr.so
(CPU: reads the gfx950 kernel metadata notes, runs nothing).  Exactly eight
k_march_tf2<GM, CU, CV> instances ship -- GM 1 / 2 (32-bit / 64-bit plane indices),
CU and CV false / true (trilinear blend / crossing combine on that axis); none uses
scratch (private segment 0, no dynamic stack, at most 256 VGPRs), and each holds the
table's 16 KiB of static LDS.  The one-plane family beside it is what it was: four
k_march_plane_tf instances of 4 KiB, and the counts the other code-object tests pin
(DESIGN.md section 23)."""
import re

from test_crossing_codeobj import _notes

TF2 = re.compile(r"^_ZN2vr11k_march_tf2ILi(\d+)ELb([01])ELb([01])EEE")
TF1 = re.compile(r"^_ZN2vr16k_march_plane_tfILi(\d+)ELb([01])EEE")


def _tf2():
    return {(int(m.group(1)), int(m.group(2)), int(m.group(3))): v for n, v in _notes().items()
            for m in [TF2.match(n or "")] if m}


def test_exactly_eight_instances_ship():
    want = {(gm, cu, cv) for gm in (1, 2) for cu in (0, 1) for cv in (0, 1)}
    assert set(_tf2()) == want, sorted(_tf2())
    names = [n for n in _notes() if n and "k_march_tf2" in n]
    assert len(names) == 8, names


def test_no_scratch_and_the_table_in_lds():
    inst = _tf2()
    assert len(inst) == 8
    bad = {k: v for k, v in inst.items()
           if v["private_segment_fixed_size"] or v["dynamic_stack"]
           or v["group_segment_fixed_size"] < 16384}
    assert not bad, bad
    assert all(1 <= v["vgpr_count"] <= 256 for v in inst.values()), \
        {k: v["vgpr_count"] for k, v in inst.items()}
    # two plane pointers, Params, the table pointer, nu, nv, v_offset, v_scale: the
    # one-plane march's arguments, one more pointer (8 bytes) and three more words
    # (12), of which 4 fill the padding after its `int n` -- 16 bytes in all, so
    # Params did not grow for this
    tf1 = [v for n, v in _notes().items() if TF1.match(n or "")]
    assert {v["kernarg_segment_size"] for v in inst.values()} == \
        {tf1[0]["kernarg_segment_size"] + 16}


def test_the_other_families_are_what_they_were():
    """the names carry no string another code-object test counts"""
    tf1 = {(int(m.group(1)), int(m.group(2))): v for n, v in _notes().items()
           for m in [TF1.match(n or "")] if m}
    assert set(tf1) == {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert len([n for n in _notes() if n and "k_march_plane_tf" in n]) == 4
    assert all(v["group_segment_fixed_size"] == 4096 and not v["private_segment_fixed_size"]
               for v in tf1.values()), tf1
    assert len({v["kernarg_segment_size"] for v in tf1.values()}) == 1
    assert len([n for n in _notes() if n and "cross" in n]) == 14
