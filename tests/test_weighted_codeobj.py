"""Code-object checks of the weighted-bin query in the built libvr.so (CPU: reads
the gfx950 kernel metadata notes, runs nothing).  Every k_march_lin<T, B> and
k_bake_lin<T, B> instance ships -- T float or _Float16, B in 1, 2, 4, 8, 16, 32 --
none uses scratch (private segment 0, no dynamic stack, at most 256 VGPRs), and
the march takes its weights as a kernel argument of their own after Params
(DESIGN.md section 16)."""
import os
import re
import subprocess
import tempfile

from test_codeobj import LIB, LLVM, MAGIC, _kernels

NAME = re.compile(r"^_ZN2vr1[01]k_(march|bake)_linI(f|DF16_)Li(\d+)EEE")
PIPE_H = re.compile(r"^_ZN2vr14k_march_pipe_hILi(\d+)ELi1ELb0EEE")
WANT = {(t, b) for t in ("f", "DF16_") for b in (1, 2, 4, 8, 16, 32)}


def _instances(kind):
    out = {}
    for name, meta in _kernels().items():
        m = NAME.match(name or "")
        if m and m.group(1) == kind:
            out[(m.group(2), int(m.group(3)))] = meta
    return out


def _kernarg_sizes():
    """kernel name -> kernarg_segment_size (test_codeobj._kernels keeps only the
    scratch and register fields of the same notes)"""
    _kernels()  # skips when the library or the LLVM tools are absent
    out = {}
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", LIB,
                        os.path.join(td, "junk")], check=True)
        data = open(fat, "rb").read()
        offs = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        for k, a in enumerate(offs):
            b = offs[k + 1] if k + 1 < len(offs) else len(data)
            part, co = os.path.join(td, f"b{k}.bin"), os.path.join(td, f"b{k}.co")
            open(part, "wb").write(data[a:b])
            r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}",
                                f"--output={co}"], capture_output=True)
            if r.returncode or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True,
                                   text=True).stdout
            for blk in notes.split("  - .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                size = re.search(r"\.kernarg_segment_size:\s+(\d+)", blk)
                if name and size:
                    out[name.group(1)] = int(size.group(1))
    return out


def test_every_weighted_instance_ships():
    march, bake = _instances("march"), _instances("bake")
    assert set(march) == WANT, sorted(WANT ^ set(march))
    assert set(bake) == WANT, sorted(WANT ^ set(bake))


def test_weighted_kernels_use_no_scratch():
    inst = {("march",) + k: v for k, v in _instances("march").items()}
    inst.update({("bake",) + k: v for k, v in _instances("bake").items()})
    assert len(inst) == 24, sorted(inst)
    bad = {k: v for k, v in inst.items() if v["private"] or v["dynamic_stack"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 256 for v in inst.values()), {k: v["vgpr"] for k, v in inst.items()}


def test_weights_are_a_kernel_argument_of_their_own():
    """vol + Params + BinWeights (32 floats) against k_march_pipe_h<B, 1>'s vol +
    Params: at least 128 bytes more, so Params itself did not grow into it"""
    ka = _kernarg_sizes()
    pipe_h = {int(PIPE_H.match(n).group(1)): s for n, s in ka.items() if PIPE_H.match(n)}
    assert set(pipe_h) == {1, 2, 4, 8, 16, 32}, sorted(pipe_h)
    seen = 0
    for name, size in ka.items():
        m = NAME.match(name)
        if m and m.group(1) == "march":
            assert size >= pipe_h[int(m.group(3))] + 128, (name, size, pipe_h)
            seen += 1
    assert seen == 12
