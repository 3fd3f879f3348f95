"""Code-object checks of the GMM quantile kernels (CPU: reads the gfx950 kernel
metadata notes of the built libvr.so and the listings kept in
profiles/gmm_quantile, runs nothing).  All 24 instances ship --
k_march_gmm_quant<K, SPREAD>, k_march_gmm_quant_h<K, SPREAD> and
k_bake_gmm_quant<T, K, SPREAD>, K in 8, 16, 32, T in float, _Float16 -- and none
uses scratch: private segment 0 and no dynamic stack.  The
listings show every kernel of the parent unchanged row for row and the 24 as the
only new rows, each with the table's 1 296 bytes of static LDS."""
import os
import re

from test_codeobj import _kernels

# vr::k_march_gmm_quant<K, SPREAD> / vr::k_march_gmm_quant_h<...> / vr::k_bake_gmm_quant<T, K, SPREAD>
MARCH = re.compile(r"^_ZN2vr\d+k_march_gmm_quant(_h)?ILi(\d+)ELb([01])EEE")
BAKE = re.compile(r"^_ZN2vr\d+k_bake_gmm_quantI(f|DF16_)Li(\d+)ELb([01])EEE")
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                        "gmm_quantile")


def _key(name):
    m = MARCH.match(name or "")
    if m:
        return ("march", "f16" if m.group(1) else "f32", int(m.group(2)), m.group(3) == "1")
    m = BAKE.match(name or "")
    if m:
        return ("bake", "f32" if m.group(1) == "f" else "f16", int(m.group(2)), m.group(3) == "1")
    return None


WANT = {(k, t, n, s) for k in ("march", "bake") for t in ("f32", "f16") for n in (8, 16, 32)
        for s in (False, True)}


def _instances():
    return {_key(name): meta for name, meta in _kernels().items() if _key(name)}


def test_every_gmm_quantile_instance_ships():
    inst = _instances()
    assert len(WANT) == 24 and set(inst) == WANT, sorted(WANT ^ set(inst))


def test_gmm_quantile_uses_no_scratch():
    inst = _instances()
    assert inst, "no GMM quantile kernel in libvr.so"
    bad = {k: v for k, v in inst.items() if v["private"] or v["dynamic_stack"]}
    assert not bad, bad


def _listing(name):
    rows = {}
    for line in open(os.path.join(PROFILES, name)):
        if line.strip() and not line.startswith("#"):
            f = line.split()
            rows[f[0]] = f[1:]
    return rows


def test_listings_parent_rows_unchanged_and_24_new():
    """columns: symbol size, vgpr_count, sgpr_count, private_segment_fixed_size,
    group_segment_fixed_size, kernarg_segment_size (tools/codeobj_list.py)"""
    parent, this = _listing("codeobj_parent.txt"), _listing("codeobj_this.txt")
    assert len(parent) > 500
    changed = {k: (v, this.get(k)) for k, v in parent.items() if this.get(k) != v}
    assert not changed, changed
    assert open(os.path.join(PROFILES, "codeobj_common.diff")).read() == ""
    new = {k: v for k, v in this.items() if k not in parent}
    assert {_key(k) for k in new} == WANT and len(new) == 24, sorted(new)
    for k, v in new.items():
        assert v[3] == "0" and v[4] == "1296", (k, v)
