"""Code-object checks of the ray projections in the built libvr.so (CPU: reads the
gfx950 kernel metadata notes, runs nothing).  Every k_march_proj<GM, CROSS, MODE>
instance ships -- GM 1 or 2 (32-bit and 64-bit plane indices), CROSS false or true,
MODE 1, 2 or 3 (maximum, minimum, mean); none uses scratch (private segment 0, no
dynamic stack, at most 256 VGPRs) or LDS -- the table is read from global memory
after the loop -- and each takes the arguments of k_march_plane_tf (DESIGN.md
section 24)."""
import re

from test_crossing_codeobj import _notes

PROJ = re.compile(r"^_ZN2vr12k_march_projILi(\d+)ELb([01])ELi(\d+)EEE")
TF = re.compile(r"^_ZN2vr16k_march_plane_tfILi(\d+)ELb([01])EEE")
WANT = {(gm, cross, mode) for gm in (1, 2) for cross in (0, 1) for mode in (1, 2, 3)}


def _proj():
    return {tuple(int(v) for v in m.groups()): meta for n, meta in _notes().items()
            for m in [PROJ.match(n or "")] if m}


def test_every_projection_instance_ships():
    proj = _proj()
    assert set(proj) == WANT, sorted(WANT ^ set(proj))
    assert len([n for n in _notes() if n and "k_march_proj" in n]) == 12


def test_projection_kernels_use_no_scratch_and_no_lds():
    proj = _proj()
    assert len(proj) == 12, sorted(proj)
    bad = {k: v for k, v in proj.items()
           if v["private_segment_fixed_size"] or v["dynamic_stack"] or v["group_segment_fixed_size"]}
    assert not bad, bad
    assert all(0 < v["vgpr_count"] <= 256 for v in proj.values()), \
        {k: v["vgpr_count"] for k, v in proj.items()}


def test_the_march_takes_the_arguments_of_k_march_plane_tf():
    """plane + Params + table + n: the kernarg segment of k_march_plane_tf<GM, CROSS>,
    byte for byte in size, so Params has not grown for the projections"""
    proj = _proj()
    tf = {(int(m.group(1)), int(m.group(2))): v for n, v in _notes().items()
          for m in [TF.match(n or "")] if m}
    assert set(tf) == {(gm, cross) for gm in (1, 2) for cross in (0, 1)}, sorted(tf)
    for key in sorted(WANT):
        assert proj[key]["kernarg_segment_size"] == tf[key[:2]]["kernarg_segment_size"] > 0, key
