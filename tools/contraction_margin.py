"""What floating-point contraction does to the reference's frames (CPU, tooling).

nvcc contracts a * b + c into a fused multiply-add by default, so the reference as
its authors ran it may have evaluated d_basicDataProcessing and d_render with
FMAs wherever the compiler found one; the oracle's canonical reading has none
(DESIGN.md section 3).  This compares two CPU builds of the reference's own kernel
text (oracle/ref/build_ref.py): -ffp-contract=off (canonical) and -ffp-contract=fast
-mfma.  gcc's choice of which products to fuse need not be nvcc's: the figures
say how far a contracted build can move, not what an NVIDIA build printed.

For the reference's shape (50 x 50 x 10 x 32), the synthetic field and a volume of
per-voxel random histograms, cameras C0 and the (30, 45) oblique view: statistic
words that differ per plane, and RGBA8 pixels that differ per method, at the
default render parameters and summed over four narrow transfer windows
(transfer_scale 256, density 0.5, across the statistic's 10th-90th percentile).
The reference writes RGBA8 only; the float figures (pixels with a float RGBA
word changed, pixels past 1e-4 in any channel) come from the saturated float
RGBA it packs, which the shim's __saturatef keeps (oracle/ref/shim/helper_cuda.h).

  python tools/contraction_margin.py [--size 512] [--json profiles/reference/contraction.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLANES = ("mean", "variance", "entropy")
DEFAULT = dict(density=0.05, brightness=1.0, transfer_offset=0.0, transfer_scale=1.0)


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512, help="frame edge (the reference's 512)")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import __graft_entry__ as g
    import magnify
    orc, R = g.load_oracle(), g.load_reference()
    off, fma = R.load("b32"), R.load("b32_fma")
    nx, ny, nz = R.DIMS
    rng = np.random.default_rng(1032)
    p = rng.random((nz, ny, nx, 32)) ** 3
    p[rng.random(p.shape) < 0.1] = 0.0
    p[..., 0] += 1e-3
    p /= magnify._total(p)
    volumes = {"synthetic field": orc.synth_volume(nx, ny, nz, 32),
               "random histograms": np.ascontiguousarray(p.astype(np.float32))}
    codec = orc.synth_codec(nx, ny, nz, 32)
    W = H = args.size
    rows = []
    for vname, vol in volumes.items():
        planes = {}
        for lib in (off, fma):
            lib.init(vol, codec)
            planes[lib.name] = lib.basic_data_processing()
        for k, kind in enumerate(("original", "fractal")):
            a, b = planes["b32"][k], planes["b32_fma"][k]
            for c, pname in enumerate(PLANES):
                d = words(a[:, c]) != words(b[:, c])
                rel = np.abs(a[d, c].astype(np.float64) - b[d, c]) / np.abs(a[d, c])
                row = dict(volume=vname, what="plane", plane=f"{kind} {pname}",
                           words=int(d.size), differ=int(d.sum()),
                           max_rel=float(rel.max()) if rel.size else 0.0)
                rows.append(row)
                print(f"{vname:18s} {kind:8s} {pname:8s}: {row['differ']:6d} of {row['words']} "
                      f"words differ, max relative {row['max_rel']:.2e}", flush=True)
        stat = {1: planes["b32"][0][:, 0], 2: planes["b32"][0][:, 1], 3: planes["b32"][0][:, 2],
                7: planes["b32"][0][:, 0] * np.float32(0.0217 * 50.0),
                4: planes["b32"][1][:, 0], 5: planes["b32"][1][:, 1], 6: planes["b32"][1][:, 2]}
        for cam in ("C0", "OBL"):
            m = magnify.camera(cam)
            for method in (1, 2, 3, 7, 4, 5, 6):
                lo, hi = magnify._p10_p90(stat[method])
                wins = [dict(density=0.5, brightness=1.0, transfer_offset=float(t),
                             transfer_scale=256.0) for t in magnify.windows(lo, hi, 4, 256.0)]
                for label, sets in (("default", [DEFAULT]), ("4 narrow windows", wins)):
                    differ = hit = fdiffer = over = 0
                    for kw in sets:
                        prm = orc.make_params(W, H, m, query_method=method, m7_dims=R.DIMS, **kw)
                        a, af = off.render(prm, prefill=0xFFFFFFFF, want_float=True)
                        b, bf = fma.render(prm, prefill=0xFFFFFFFF, want_float=True)
                        h = ~np.isnan(af).any(axis=-1)
                        assert np.array_equal(h, ~np.isnan(bf).any(axis=-1))  # same rays hit
                        differ += int(np.sum(a != b))
                        hit += int(h.sum())
                        fdiffer += int(np.sum(np.any(words(af[h]) != words(bf[h]), axis=-1)))
                        over += int(np.sum(np.any(np.abs(af[h] - bf[h]) > 1e-4, axis=-1)))
                    rows.append(dict(volume=vname, what="frame", camera=cam, method=method,
                                     parameters=label, frame=f"{W}x{H}", hit=hit,
                                     rgba8_differ=differ, float_words_differ=fdiffer,
                                     over_1e4=over, over_1e4_share=over / hit))
                    print(f"{vname:18s} {cam:3s} m{method} {label:16s}: of {hit} hit pixels "
                          f"{differ:6d} differ in RGBA8, {fdiffer:7d} in a float word, "
                          f"{over:6d} ({100.0 * over / hit:.2f} %) past 1e-4", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(args.json), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
