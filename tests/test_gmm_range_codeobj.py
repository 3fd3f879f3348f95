"""Code-object checks of the GMM range-probability kernels in the built libvr.so
(CPU: reads the gfx950 kernel metadata notes, runs nothing).  All twelve
instances ship -- k_march_gmm_range<K>, k_march_gmm_range_h<K> and
k_bake_gmm_range<T, K>, K in 8, 16, 32, T in float, _Float16 -- and none uses
scratch: private segment 0 and no dynamic stack."""
import re

from test_codeobj import _kernels

# vr::k_march_gmm_range<K> / vr::k_march_gmm_range_h<K> / vr::k_bake_gmm_range<T, K>
MARCH = re.compile(r"^_ZN2vr\d+k_march_gmm_range(_h)?ILi(\d+)EEE")
BAKE = re.compile(r"^_ZN2vr\d+k_bake_gmm_rangeI(f|DF16_)Li(\d+)EEE")


def _instances():
    out = {}
    for name, meta in _kernels().items():
        m = MARCH.match(name or "")
        if m:
            out[("march", "f16" if m.group(1) else "f32", int(m.group(2)))] = meta
        m = BAKE.match(name or "")
        if m:
            out[("bake", "f32" if m.group(1) == "f" else "f16", int(m.group(2)))] = meta
    return out


def test_every_gmm_range_instance_ships():
    inst = _instances()
    want = {(k, t, n) for k in ("march", "bake") for t in ("f32", "f16") for n in (8, 16, 32)}
    assert set(inst) == want, sorted(want ^ set(inst))


def test_gmm_range_uses_no_scratch():
    inst = _instances()
    assert inst, "no GMM range kernel in libvr.so"
    bad = {k: v for k, v in inst.items() if v["private"] or v["dynamic_stack"]}
    assert not bad, bad
