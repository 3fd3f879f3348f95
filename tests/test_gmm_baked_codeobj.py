"""Code-object checks of the GMM bake kernel in the built libvr.so (CPU: reads the
gfx950 kernel metadata notes, runs nothing).  Every k_bake_gmm<T, K> instance
ships -- T in float, _Float16; K in 8, 16, 32 -- and none uses scratch: private
segment 0 and no dynamic stack."""
import re

from test_codeobj import _kernels

# vr::k_bake_gmm<float, K> / <_Float16, K>
NAME = re.compile(r"^_ZN2vr10k_bake_gmmI(f|DF16_)Li(\d+)EEE")


def _instances():
    out = {}
    for name, meta in _kernels().items():
        m = NAME.match(name or "")
        if m:
            out[("f32" if m.group(1) == "f" else "f16", int(m.group(2)))] = meta
    return out


def test_every_gmm_bake_instance_ships():
    inst = _instances()
    want = {(t, k) for t in ("f32", "f16") for k in (8, 16, 32)}
    assert set(inst) == want, sorted(want ^ set(inst))


def test_gmm_bake_uses_no_scratch():
    inst = _instances()
    assert inst, "no k_bake_gmm instance in libvr.so"
    bad = {k: v for k, v in inst.items() if v["private"] or v["dynamic_stack"]}
    assert not bad, bad
