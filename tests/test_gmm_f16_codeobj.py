"""Code-object checks of the f16 GMM march in the built libvr.so (CPU: reads the
gfx950 kernel metadata notes, runs nothing).  Every k_march_gmm_h<K, M, COUNT>
instance ships -- K in 8, 16, 32, M in 1, 2, rendering and footprint-counting
-- and none uses scratch: private segment 0, no dynamic stack, at most 256
VGPRs."""
import re

from test_codeobj import _kernels

NAME = re.compile(r"^_ZN2vr13k_march_gmm_hILi(\d+)ELi(\d+)ELb([01])EEE")


def _instances():
    out = {}
    for name, meta in _kernels().items():
        m = NAME.match(name or "")
        if m:
            out[(int(m.group(1)), int(m.group(2)), m.group(3) == "1")] = meta
    return out


def test_every_f16_gmm_march_instance_ships():
    inst = _instances()
    want = {(k, m, c) for k in (8, 16, 32) for m in (1, 2) for c in (False, True)}
    assert set(inst) == want, sorted(want ^ set(inst))
    assert len(inst) == 12


def test_f16_gmm_marches_use_no_scratch():
    inst = _instances()
    assert inst, "no k_march_gmm_h instance in libvr.so"
    bad = {k: v for k, v in inst.items() if v["private"] or v["dynamic_stack"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 256 for v in inst.values()), {k: v["vgpr"] for k, v in inst.items()}
