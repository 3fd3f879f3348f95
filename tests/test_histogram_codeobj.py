"""Code-object checks of the plane histogram and range kernels in the built libvr.so
(CPU: reads the gfx950 kernel metadata notes, runs nothing and searches no
instructions).  Both k_plane_hist instances (V = 0: one plane, V = 1: two) and the
one k_plane_range ship; none uses scratch (private segment 0, no dynamic stack); the
histogram's LDS is all dynamic (no static group segment), the range kernel has none;
and the kernel-argument bytes are the figures of DESIGN.md section 27.2: k_plane_hist
two plane pointers, the 72-byte walk (two 64-bit pitches and fourteen 32-bit words),
four window floats, nu, nv, the replication's log2, padding, and the pointer of the
counts; k_plane_range one pointer, the walk, and the pointers of the keys and of the
NaN count."""
import re

from test_crossing_codeobj import _notes

HIST = re.compile(r"^_ZN2vr12k_plane_histILi(\d+)EEE")
WALK_BYTES = 2 * 8 + 14 * 4                                   # 72
HIST_KERNARG_BYTES = 8 + 8 + WALK_BYTES + 4 * 4 + 3 * 4 + 4 + 8   # 128
RANGE_KERNARG_BYTES = 8 + WALK_BYTES + 8 + 8                  # 96


def _hist():
    return {int(m.group(1)): v for n, v in _notes().items() for m in [HIST.match(n or "")] if m}


def _range():
    return {n: v for n, v in _notes().items() if n and "k_plane_range" in n}


def test_both_histogram_instances_and_the_range_kernel_ship():
    assert sorted(_hist()) == [0, 1], sorted(_hist())
    assert len(_range()) == 1, sorted(_range())


def test_no_scratch_and_the_stated_lds_and_kernarg_bytes():
    for v, meta in _hist().items():
        assert meta["private_segment_fixed_size"] == 0 and not meta["dynamic_stack"], (v, meta)
        assert meta["group_segment_fixed_size"] == 0, (v, meta)  # sized at launch from nu * nv
        assert meta["kernarg_segment_size"] == HIST_KERNARG_BYTES == 128, (v, meta)
        assert 0 < meta["vgpr_count"] <= 64, (v, meta)  # 8 waves per SIMD: two workgroups per CU
    (name, meta), = _range().items()
    assert meta["private_segment_fixed_size"] == 0 and not meta["dynamic_stack"], meta
    assert meta["group_segment_fixed_size"] == 0, meta
    assert meta["kernarg_segment_size"] == RANGE_KERNARG_BYTES == 96, meta
    assert 0 < meta["vgpr_count"] <= 64, meta
