"""Code-object checks of the gradient bake in the built libvr.so (CPU: reads the
gfx950 kernel metadata notes, runs nothing and searches no instructions).  The one
k_bake_grad ships; it uses no scratch (private segment 0, no dynamic stack), and its
LDS and kernel-argument bytes are the figures of DESIGN.md section 26.2: two tiles
of 18 rows x 63 columns of floats (the double-buffered slice with its halo), and two
pointers, two 64-bit pitches, three dimensions and the pointer of the maximum."""
from test_crossing_codeobj import _notes

LDS_BYTES = 2 * 18 * 63 * 4      # 9072
KERNARG_BYTES = 8 + 8 + 8 + 8 + 4 + 4 + 4 + 4 + 8  # 56 (the padding before the last pointer too)


def _grad():
    return {n: v for n, v in _notes().items() if n and "k_bake_grad" in n}


def test_the_one_instance_ships():
    assert len(_grad()) == 1, sorted(_grad())


def test_no_scratch_and_the_stated_lds_and_kernarg_bytes():
    (name, v), = _grad().items()
    assert v["private_segment_fixed_size"] == 0 and not v["dynamic_stack"], v
    assert v["group_segment_fixed_size"] == LDS_BYTES == 9072, v
    assert v["kernarg_segment_size"] == KERNARG_BYTES == 56, v
    assert 0 < v["vgpr_count"] <= 64, v  # 8 waves per SIMD: two workgroups of 1024 per CU
