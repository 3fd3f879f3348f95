#!/usr/bin/env python3
"""Record which march kernel renders each case of the kernel-choice table.

For every case (volume shape, bins, method, dtype, baked or not, view, frame,
tile list, knobs) one frame is rendered through the public Python API and one
line is written: the case key, then last_kernel().  tests/golden/kernel_choice.txt
is this tool's output at the commit before the choice moved into csrc/vr_plan.cpp;
tests/test_plan.py replays the keys through plan_march() on the CPU
(tests/c/plancheck.cpp) and compares the names.

    python tools/record_kernel_choice.py OUT.txt

File format.  '@vol NAME nx ny nz', '@view NAME m0 m4 m8' (the three entries of
the inverse view matrix the choice reads) and '@frame NAME W H' lines define
the names; every other line is

    VOL NB METHOD FLAGS VIEW FRAME TILES KNOBS KERNEL

FLAGS: '-' or any of h (f16 records), b (baked: bake_stats() was called),
a (adopted, not owned), z (layout budget 0: no layout copy can be made),
g (method-7 grid different from the volume).  TILES: '-' (full frame) or the
number of tiles of the tile list.  KNOBS: '-' or KEY=VALUE[,KEY=VALUE...].
"""
from __future__ import annotations

import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOLS = {
    "A": (48, 48, 48),      # coarse for every frame (4 * face <= 256^2 on all three faces)
    "B": (768, 768, 8),     # x-y face fine up to 1080p, x-z and y-z faces coarse
    "C": (64, 64, 2048),    # x-y face coarse; x-z / y-z faces fine up to 640^2, coarse above
    "D": (256, 256, 8),     # x-y face fine at 256^2, coarse from 512^2
}
FRAMES = {"1": (256, 256), "2": (512, 512), "3": (640, 640), "4": (768, 768), "5": (1920, 1080)}
# (rx, ry) of camera.display_inv_view; R is the runSingleTest view
ROTS = {"R": None, "O": (30.0, 45.0), "S": (0.0, 90.0), "T": (90.0, 90.0),
        "r": (0.0, 19.0), "s": (0.0, 71.0), "t": (90.0, 71.0)}
M7_GRID = (10, 12, 20)
NBS = (1, 2, 4, 8, 16, 32)


def cases():
    """Every case as (vol, nb, method, flags, view, frame, tiles, knobs)."""
    out = []

    def add(vol, nb, m, flags, view, frame, tiles=0, knobs=""):
        if "h" in flags and m == 7 and "b" not in flags:
            return  # rejected: f16 method 7 reads the baked corner means
        c = (vol, nb, m, "".join(sorted(flags)), view, frame, tiles, knobs)
        if c not in seen:
            seen.add(c)
            out.append(c)

    seen = set()
    views, frames = "ROSTrst", "12345"
    # fp32 records, per-step decode: the whole cross product on the coarse and the fine volume
    # (the views just under 0.95 at the smallest and the largest frame)
    for vol, nb, m, v, f in itertools.product("AB", NBS, (1, 2, 3, 7), views, frames):
        if v in "ROST" or f in "15":
            add(vol, nb, m, "", v, f)
    # the face test of side / top views, the mid-size x-y test
    for nb, m, v, f in itertools.product((1, 2, 4, 8), (1, 2, 3), "ST", frames):
        add("C", nb, m, "", v, f)
    for nb, m, v, f in itertools.product((1, 4, 8, 16), (1, 2, 3), "RO", frames):
        add("D", nb, m, "", v, f)
    # baked planes
    for vol, nb, m, v, f in itertools.product("AB", (1, 8), (1, 2, 3, 7), views, "15"):
        add(vol, nb, m, "b", v, f)
    # f16 records
    for nb, m, v, f in itertools.product(NBS, (1, 2, 3), "ROS", "15"):
        add("A", nb, m, "h", v, f)
    for nb, m, v in itertools.product((1, 8), (1, 2, 3, 7), "ROST"):
        add("A", nb, m, "bh", v, "5")
    for m, v in itertools.product((1, 3), "ROS"):
        add("B", 8, m, "h", v, "5")
        add("B", 8, m, "bh", v, "5")
    # method 7 on a grid that is not the volume's
    for vol, nb, v, f in itertools.product("AB", NBS, "RO", "5"):
        add(vol, nb, 7, "g", v, f)
    for v in "RO":
        add("A", 8, 7, "bg", v, "5")
    # adopted volumes (no axis copy), denied layout copies
    for vol, nb, m, v, f in itertools.product("AB", (4, 8), (1, 2, 3, 7), "ROST", "5"):
        add(vol, nb, m, "a", v, f)
    for vol, nb, m, b, v, f in itertools.product("AB", (4, 8), (1, 2, 3, 7), ("", "b"), "OST", "15"):
        add(vol, nb, m, "z" + b, v, f)
    # tile lists at 1080p, n_tiles * 256 on each side of 400 000 and 700 000
    tl = (1562, 1563, 2734, 2735)
    for vol, nb, m, v, t in itertools.product("B", NBS, (1, 2, 3, 7), "ROS", tl):
        add(vol, nb, m, "", v, "5", t)
    for nb, m, v, t in itertools.product((1, 8, 16), (1, 2, 3, 7), "RO", (1562, 2735)):
        add("A", nb, m, "", v, "5", t)
    for nb, m, v, t in itertools.product((4, 8), (1, 2), "Tt", tl):
        add("B", nb, m, "", v, "5", t)
    for nb, m, v, t in itertools.product((1, 8), (1, 2, 7), "ROS", tl):
        add("B", nb, m, "b", v, "5", t)
    for m, v, t in itertools.product((1, 3), "RO", (1562, 2735)):
        add("A", 8, m, "h", v, "5", t)
    for m, v, t in itertools.product((1, 2), "OS", (1562, 2735)):
        add("B", 8, m, "z", v, "5", t)
        add("B", 8, m, "a", v, "5", t)

    # knobs, each on the cases it can affect
    def knob(keys, values, base):
        for val in values:
            k = ",".join(f"{key}={v}" for key, v in zip(keys, val if isinstance(val, tuple) else (val,)))
            for b in base:
                add(b[0], b[1], b[2], b[3], b[4], b[5], b[6] if len(b) > 6 else 0, k)

    F = "5"
    knob(["VR_PATH"], (0, 1, 2, 4, 7, 3),
         [("A", 8, 1, "", "R", F), ("B", 8, 1, "", "O", F), ("B", 8, 3, "", "R", F),
          ("A", 4, 2, "", "O", "2"), ("B", 16, 1, "", "R", F), ("B", 32, 3, "", "O", F),
          ("B", 16, 3, "", "R", F), ("B", 8, 1, "", "S", F), ("B", 2, 3, "", "R", F),
          ("B", 1, 1, "", "O", F), ("B", 8, 1, "b", "O", F), ("B", 8, 2, "b", "R", F),
          ("B", 8, 1, "b", "S", F), ("B", 8, 7, "", "O", F), ("B", 8, 1, "", "R", F, 1562),
          ("B", 8, 1, "", "O", F, 1562), ("B", 8, 1, "b", "R", F, 1562)])
    knob(["VR_SEG"], (2, 4, -2, -4, 3),
         [("B", 8, 1, "", "R", F, 1562), ("B", 8, 1, "", "S", F, 1562), ("B", 8, 2, "", "T", F, 2734),
          ("A", 1, 1, "", "R", "1"), ("A", 4, 1, "", "O", "2"), ("A", 8, 2, "", "O", F),
          ("B", 8, 1, "b", "O", F), ("B", 8, 1, "b", "R", F, 1562), ("B", 8, 1, "b", "S", F),
          ("A", 1, 3, "", "R", "1")])
    knob(["VR_PATH", "VR_SEG"], ((7, 2), (7, 4), (7, -2), (7, -4)),
         [("B", 8, 3, "", "R", F), ("B", 16, 1, "", "R", F), ("B", 32, 3, "", "O", F),
          ("B", 4, 1, "", "S", F), ("B", 1, 1, "b", "R", F), ("B", 8, 7, "", "R", F)])
    knob(["VR_DUO"], (0, 1, 2, 3, 4),
         [("A", 8, 1, "", "R", F), ("A", 8, 2, "", "R", F), ("A", 4, 1, "", "R", "2"),
          ("A", 8, 3, "", "R", F), ("A", 16, 1, "", "R", F), ("B", 8, 1, "", "R", F)])
    knob(["VR_PATH", "VR_DUO"], ((1, 0), (1, 2), (1, 3), (1, 4)),
         [("B", 8, 1, "", "R", F), ("B", 4, 2, "", "O", F), ("B", 16, 2, "", "R", F)])
    knob(["VR_DUO", "VR_BOX_MAX"], ((2, 0), (4, 1024)), [("A", 8, 1, "", "R", F)])
    knob(["VR_WIDE"], (1, 2, 3),
         [("B", 16, 1, "", "R", F), ("B", 16, 1, "", "O", F), ("B", 32, 1, "", "R", F),
          ("B", 16, 3, "", "O", F), ("B", 32, 2, "", "O", F), ("B", 16, 2, "", "S", F, 1562)])
    knob(["VR_QUAD2"], (0, 1),
         [("B", 8, 1, "", "O", F), ("B", 8, 1, "", "O", F, 1562), ("B", 8, 3, "", "O", F, 2735),
          ("B", 8, 2, "z", "O", F, 1562), ("B", 8, 2, "z", "O", F)])
    heads = [("B", 8, 1, "", "R", F, 1562), ("B", 8, 2, "", "S", F, 1562),
             ("B", 8, 1, "", "T", F, 1563), ("B", 8, 1, "", "R", F, 2734), ("B", 4, 1, "", "R", F, 1562)]
    knob(["VR_HEAD"], (0, 32, 64, 68, 2000), heads)
    knob(["VR_HEAD_SEG"], (-2, -4, -8, -3), heads)
    knob(["VR_HEAD_TAIL"], (0, 1), heads)
    knob(["VR_HEAD_TAIL", "VR_HEAD_SEG"], ((1, -2), (1, -8)), heads)
    knob(["VR_HEAD", "VR_SEG"], ((64, -4), (64, 4)), heads)
    knob(["VR_ZROWS"], (0,),
         [("B", 8, 1, "", "S", F), ("B", 4, 2, "", "T", F), ("A", 8, 1, "", "S", F),
          ("B", 8, 3, "", "S", F), ("A", 2, 3, "", "T", "1"), ("B", 8, 1, "", "S", F, 1562)])
    knob(["VR_BOX3"], (0, 1),
         [("A", 16, 3, "", "R", F), ("A", 32, 3, "", "R", F), ("B", 16, 3, "", "R", F),
          ("A", 32, 3, "", "O", F)])
    knob(["VR_BOX_MAX"], (0, 4096), [("A", 8, 1, "", "R", F), ("A", 8, 3, "", "R", F)])
    knob(["VR_SEG_RAYS"], (0, 100000, 3000000),
         [("A", 8, 1, "", "R", F), ("A", 1, 1, "", "R", "1"), ("B", 8, 1, "", "R", F, 2735),
          ("A", 4, 1, "", "O", "3"), ("A", 16, 3, "", "R", "4"), ("A", 32, 1, "", "R", F),
          ("A", 2, 3, "", "R", "2"), ("A", 8, 2, "", "S", F)])
    knob(["VR_PLANE_WIDE"], (0, 1),
         [("A", 8, 1, "b", "R", "1"), ("A", 8, 2, "b", "O", "1"), ("A", 8, 1, "b", "S", "1"),
          ("A", 8, 3, "bz", "S", "1"), ("A", 8, 7, "b", "R", "1")])
    knob(["VR_M7_QUAD"], (0, 1), [("A", 8, 7, "", "O", F), ("B", 8, 7, "", "O", F),
                                  ("B", 8, 7, "z", "O", F)])
    knob(["VR_M7_WQ"], (0, 1), [("A", 16, 7, "", "R", F), ("A", 32, 7, "", "O", F)])
    knob(["VR_M7_PIPE"], (0, 1), [("A", 8, 7, "", "R", F), ("A", 4, 7, "", "O", F),
                                  ("A", 8, 7, "g", "O", F)])
    knob(["VR_M7_QUAD", "VR_M7_PIPE"], ((0, 0),), [("B", 8, 7, "", "O", F)])
    knob(["VR_WG_PER_CU"], (3, 0, 33),
         [("B", 8, 1, "", "O", F), ("B", 8, 7, "", "O", F), ("B", 8, 1, "b", "O", F),
          ("B", 8, 7, "b", "R", F), ("A", 8, 1, "", "R", F), ("B", 8, 1, "", "O", F, 1562)])
    knob(["VR_SEG_MAP"], (0, 1), [("A", 1, 1, "", "R", "1"), ("B", 8, 1, "b", "O", F),
                                  ("B", 2, 3, "", "R", F), ("A", 2, 3, "h", "R", F)])
    knob(["VR_WQ_MAP"], (0,), [("B", 32, 1, "", "O", F), ("A", 32, 7, "", "O", F)])
    knob(["VR_WIDE_MAP"], (0,), [("B", 16, 1, "", "R", F)])
    knob(["VR_BOX_MAP"], (0,), [("A", 8, 1, "", "R", F), ("A", 8, 3, "", "R", F)])
    knob(["VR_M7_MAP"], (0, 1), [("A", 8, 7, "", "R", F), ("B", 8, 7, "", "R", F)])
    return out


def key_of(c):
    vol, nb, m, flags, view, frame, tiles, knobs = c
    return f"{vol} {nb} {m} {flags or '-'} {view} {frame} {tiles or '-'} {knobs or '-'}"


def view_matrices(pkg):
    ms = {}
    for name, rot in ROTS.items():
        ms[name] = (pkg.camera.single_test_inv_view() if rot is None
                    else pkg.camera.display_inv_view(rot))
    a = {k: [abs(float(v[i])) for i in (0, 4, 8)] for k, v in ms.items()}
    assert a["R"][0] >= 0.95 and a["S"][2] >= 0.95 and a["T"][1] >= 0.95
    assert max(a["O"]) < 0.95
    assert 0.9 < a["r"][0] < 0.95 and 0.9 < a["s"][2] < 0.95 and 0.9 < a["t"][1] < 0.95
    assert max(a["r"][1:]) < 0.9 and max(a["s"][:2]) < 0.9 and max(a["t"][0], a["t"][2]) < 0.9
    return ms


def main():
    import torch
    import __graft_entry__ as ge

    out_path = sys.argv[1] if len(sys.argv) > 1 else "kernel_choice.txt"
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "the recording needs a GPU"
    torch.cuda.set_device(0)
    ms = view_matrices(pkg)
    all_cases = cases()

    max_tiles = max(c[6] for c in all_cases)
    tile_list = torch.full((max_tiles + 64,), -1, dtype=torch.int32, device="cuda")  # -1 = PAD
    tile_list[:max_tiles] = torch.arange(max_tiles, dtype=torch.int32, device="cuda")
    n_px = max(max(w * h for w, h in FRAMES.values()), (max_tiles + 64) * 256)
    out = torch.zeros(n_px, dtype=torch.int32, device="cuda")

    lines = [f"@vol {k} {v[0]} {v[1]} {v[2]}" for k, v in VOLS.items()]
    lines += [f"@view {k} {float(m[0]):.9g} {float(m[4]):.9g} {float(m[8]):.9g}" for k, m in ms.items()]
    lines += [f"@frame {k} {v[0]} {v[1]}" for k, v in FRAMES.items()]

    # one resident volume per (volume, bins, f16, adopted); baked and budget states inside
    def state(c):
        return (c[0], c[1], "h" in c[3], "a" in c[3])

    results = {}
    for st in sorted(set(state(c) for c in all_cases)):
        vol, nb, half, adopted = st
        nx, ny, nz = VOLS[vol]
        pkg.freeCudaBuffers()
        pkg.clear_tuning()
        pkg.set_layout_budget(None)
        keep = None
        if adopted:
            keep = torch.full((nz, ny, nx, nb), 1.0 / nb, dtype=torch.float32, device="cuda")
            pkg.init_distribution(keep, adopt=True)
        else:
            pkg.synthesize((nx, ny, nz), nb)
            if half:
                pkg.convert_f16()
        mine = [c for c in all_cases if state(c) == st]
        # per-step decode first, then baked; inside each, default budget then budget 0
        mine.sort(key=lambda c: ("b" in c[3], "z" in c[3]))
        baked = False
        budget0 = False
        for c in mine:
            _, _, m, flags, view, frame, tiles, knobs = c
            if "b" in flags and not baked:
                pkg.bake_stats()
                baked = True
            if ("z" in flags) != budget0:
                budget0 = "z" in flags
                pkg.set_layout_budget(0 if budget0 else None)
            pkg.clear_tuning()
            for kv in knobs.split(","):
                if kv:
                    k, v = kv.split("=")
                    pkg.set_tuning(k, v)
            W, H = FRAMES[frame]
            d = pkg.make_desc(out, W, H, ms[view], query_method=m,
                              volume_size=M7_GRID if "g" in flags else (nx, ny, nz),
                              d_tile_list=tile_list if tiles else None, n_tiles=tiles)
            pkg.render(d)
            torch.cuda.synchronize()
            results[c] = pkg.last_kernel()
        del keep
    pkg.clear_tuning()
    pkg.set_layout_budget(None)
    pkg.freeCudaBuffers()
    lines += [f"{key_of(c)} {results[c]}" for c in all_cases]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(all_cases)} cases -> {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--list":
        for c in cases():
            print(key_of(c))
    else:
        main()
