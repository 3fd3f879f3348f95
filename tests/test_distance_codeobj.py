"""Code-object checks of the distribution-distance query in the built libvr.so
(CPU: reads the gfx950 kernel metadata notes, runs nothing).  Every
k_march_dist<T, B, METRIC> and k_bake_dist<T, B, METRIC> instance ships -- T float
or _Float16, B in 1, 2, 4, 8, 16, 32, METRIC 0 (L1), 1 (EMD), 2 (KS) -- none uses
scratch (private segment 0, no dynamic stack, at most 256 VGPRs), and the march
takes its target and similarity flag as a kernel argument of their own after
Params."""
import re

from test_codeobj import _kernels
from test_weighted_codeobj import PIPE_H, _kernarg_sizes

NAME = re.compile(r"^_ZN2vr1[12]k_(march|bake)_distI(f|DF16_)Li(\d+)ELi([012])EEE")
WANT = {(t, b, k) for t in ("f", "DF16_") for b in (1, 2, 4, 8, 16, 32) for k in (0, 1, 2)}


def _instances(kind):
    out = {}
    for name, meta in _kernels().items():
        m = NAME.match(name or "")
        if m and m.group(1) == kind:
            out[(m.group(2), int(m.group(3)), int(m.group(4)))] = meta
    return out


def test_every_distance_instance_ships():
    march, bake = _instances("march"), _instances("bake")
    assert set(march) == WANT, sorted(WANT ^ set(march))
    assert set(bake) == WANT, sorted(WANT ^ set(bake))


def test_distance_kernels_use_no_scratch():
    inst = {("march",) + k: v for k, v in _instances("march").items()}
    inst.update({("bake",) + k: v for k, v in _instances("bake").items()})
    assert len(inst) == 72, sorted(inst)
    bad = {k: v for k, v in inst.items() if v["private"] or v["dynamic_stack"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 256 for v in inst.values()), {k: v["vgpr"] for k, v in inst.items()}


def test_the_target_is_a_kernel_argument_of_its_own():
    """vol + Params + DistTarget (32 floats and the flag: 33 words) against
    k_march_pipe_h<B, 1>'s vol + Params: larger, and by no more than the 33 words
    and their padding to 8 bytes, so Params itself did not grow"""
    ka = _kernarg_sizes()
    pipe_h = {int(PIPE_H.match(n).group(1)): s for n, s in ka.items() if PIPE_H.match(n)}
    assert set(pipe_h) == {1, 2, 4, 8, 16, 32}, sorted(pipe_h)
    seen = 0
    for name, size in ka.items():
        m = NAME.match(name)
        if m and m.group(1) == "march":
            base = pipe_h[int(m.group(3))]
            assert base + 4 * 33 <= size <= base + 4 * 33 + 4, (name, size, base)
            seen += 1
    assert seen == 36
