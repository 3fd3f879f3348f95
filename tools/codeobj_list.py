#!/usr/bin/env python3
"""List every gfx950 kernel of a libvr.so (tooling; CPU only, runs nothing).

One row per kernel, sorted by name: symbol size, vgpr_count, sgpr_count,
private_segment_fixed_size, group_segment_fixed_size, kernarg_segment_size -- the
listing kept in profiles/*/codeobj_*.txt to show that a change left the existing
code objects as they were.  The code objects are extracted as tests/test_codeobj.py
extracts them.

  python tools/codeobj_list.py path/to/libvr.so > listing.txt
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "kernarg_segment_size")


def kernels(lib):
    rows = {}
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib,
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
            sizes = {}
            syms = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "-W", co], capture_output=True,
                                  text=True).stdout
            for line in syms.splitlines():
                f = line.split()
                if len(f) == 8 and f[3] == "FUNC":
                    sizes[f[7]] = int(f[2])
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True,
                                   text=True).stdout
            for blk in notes.split("  - .agpr_count")[1:]:
                def get(key):
                    m = re.search(rf"\.{key}:\s+(\S+)", blk)
                    return m.group(1) if m else "0"
                name = get("name")
                rows[name] = [str(sizes.get(name, 0))] + [get(k) for k in KEYS]
    return rows


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    print("# kernel  symbol_size " + " ".join(KEYS))
    for name, row in sorted(kernels(sys.argv[1]).items()):
        print(name, *row)


if __name__ == "__main__":
    main()
