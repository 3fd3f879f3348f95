"""Code-object checks of the f16 march in the built libvr.so (CPU: reads the
gfx950 kernel metadata notes, runs nothing).  Every k_march_pipe_h<B, M, COUNT>
instance ships -- B in 1, 2, 4, 8, 16, 32, M in 1, 2, 3, rendering and
footprint-counting -- and none uses scratch: private segment 0, no dynamic
stack, at most 256 VGPRs."""
import re

from test_codeobj import _kernels

NAME = re.compile(r"^_ZN2vr14k_march_pipe_hILi(\d+)ELi(\d+)ELb([01])EEE")


def _instances():
    out = {}
    for name, meta in _kernels().items():
        m = NAME.match(name or "")
        if m:
            out[(int(m.group(1)), int(m.group(2)), m.group(3) == "1")] = meta
    return out


def test_every_f16_march_instance_ships():
    inst = _instances()
    want = {(b, m, c) for b in (1, 2, 4, 8, 16, 32) for m in (1, 2, 3) for c in (False, True)}
    assert set(inst) == want, sorted(want ^ set(inst))
    assert sum(1 for k in inst if not k[2]) == 18


def test_f16_marches_use_no_scratch():
    inst = _instances()
    assert inst, "no k_march_pipe_h instance in libvr.so"
    bad = {k: v for k, v in inst.items() if v["private"] or v["dynamic_stack"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 256 for v in inst.values()), {k: v["vgpr"] for k, v in inst.items()}
