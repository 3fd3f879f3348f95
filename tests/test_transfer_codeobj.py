"""Code-object checks of the transfer-function plane march in the built libvr.so
(CPU: reads the gfx950 kernel metadata notes, runs nothing).  Exactly four
k_march_plane_tf<GM, CROSS> instances ship -- GM 1 / 2 (32-bit / 64-bit plane
indices), CROSS false / true (trilinear blend / crossing combine); none uses scratch
(private segment 0, no dynamic stack, at most 256 VGPRs), and each holds the
table's 4 KiB of static LDS."""
import re

from test_crossing_codeobj import _notes

TF = re.compile(r"^_ZN2vr16k_march_plane_tfILi(\d+)ELb([01])EEE")


def _tf():
    return {(int(m.group(1)), int(m.group(2))): v for n, v in _notes().items()
            for m in [TF.match(n or "")] if m}


def test_exactly_four_instances_ship():
    assert set(_tf()) == {(1, 0), (1, 1), (2, 0), (2, 1)}, sorted(_tf())
    names = [n for n in _notes() if n and "k_march_plane_tf" in n]
    assert len(names) == 4, names


def test_no_scratch_and_the_table_in_lds():
    inst = _tf()
    assert len(inst) == 4
    bad = {k: v for k, v in inst.items()
           if v["private_segment_fixed_size"] or v["dynamic_stack"]
           or v["group_segment_fixed_size"] < 4096}
    assert not bad, bad
    assert all(1 <= v["vgpr_count"] <= 256 for v in inst.values()), \
        {k: v["vgpr_count"] for k, v in inst.items()}
