"""Code-object checks of the level-crossing query in the built libvr.so (CPU: reads
the gfx950 kernel metadata notes, runs nothing).  Every k_march_cross<T, B>
instance ships -- T float or _Float16, B in 1, 2, 4, 8, 16, 32 -- with both
k_march_cross_plane instances (32-bit and 64-bit plane indices); none uses scratch
(private segment 0, no dynamic stack, at most 256 VGPRs) or LDS; each march takes
the arguments of k_march_lin, and there is no bake kernel of its own (the plane of
F is k_bake_lin's)."""
import functools
import os
import re
import subprocess
import tempfile

from test_codeobj import LIB, LLVM, MAGIC, _kernels

MARCH = re.compile(r"^_ZN2vr13k_march_crossI(f|DF16_)Li(\d+)EEE")
PLANE = re.compile(r"^_ZN2vr19k_march_cross_planeILi(\d+)EEE")
LIN = re.compile(r"^_ZN2vr11k_march_linI(f|DF16_)Li(\d+)EEE")
WANT = {(t, b) for t in ("f", "DF16_") for b in (1, 2, 4, 8, 16, 32)}
KEYS = ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "kernarg_segment_size")


@functools.lru_cache(maxsize=None)
def _notes():
    """kernel name -> {key: int} and uses_dynamic_stack, of every gfx950 kernel"""
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
                def get(key):
                    m = re.search(rf"\.{key}:\s+(\S+)", blk)
                    return m.group(1) if m else None
                meta = {key: int(get(key) or 0) for key in KEYS}
                meta["dynamic_stack"] = get("uses_dynamic_stack") == "true"
                out[get("name")] = meta
    return out


def _cross():
    march = {(m.group(1), int(m.group(2))): v for n, v in _notes().items()
             for m in [MARCH.match(n or "")] if m}
    plane = {int(m.group(1)): v for n, v in _notes().items() for m in [PLANE.match(n or "")] if m}
    return march, plane


def test_every_crossing_instance_ships():
    march, plane = _cross()
    assert set(march) == WANT, sorted(WANT ^ set(march))
    assert set(plane) == {1, 2}, sorted(plane)  # gather8 MODE 1 and MODE 2


def test_crossing_kernels_use_no_scratch_and_no_lds():
    march, plane = _cross()
    inst = {("march",) + k: v for k, v in march.items()}
    inst.update({("plane", k): v for k, v in plane.items()})
    assert len(inst) == 14, sorted(inst)
    bad = {k: v for k, v in inst.items()
           if v["private_segment_fixed_size"] or v["dynamic_stack"] or v["group_segment_fixed_size"]}
    assert not bad, bad
    assert all(0 < v["vgpr_count"] <= 256 for v in inst.values()), \
        {k: v["vgpr_count"] for k, v in inst.items()}


def test_the_march_takes_the_arguments_of_k_march_lin():
    """vol + Params + BinWeights: the kernarg segment of k_march_lin<T, B>, byte for
    byte in size, so neither Params nor the weights grew for this query"""
    march, _ = _cross()
    lin = {(m.group(1), int(m.group(2))): v for n, v in _notes().items()
           for m in [LIN.match(n or "")] if m}
    assert set(lin) == WANT, sorted(lin)
    for key in sorted(WANT):
        assert march[key]["kernarg_segment_size"] == lin[key]["kernarg_segment_size"] > 0, key


def test_there_is_no_bake_kernel_of_its_own():
    names = [n for n in _notes() if n and "cross" in n]
    assert len(names) == 14, names
    assert not [n for n in _notes() if n and "k_bake_cross" in n]
