#!/usr/bin/env python3
"""k_march_cross against k_march_lin under VR_WG_PER_CU caps (tooling; DESIGN.md
section 21.4): do the workgroups per CU that the two kernels' register counts allow
explain a difference between them?

The 1024^3 x 8 scene of tools/bench_crossing.py, all weights zero (identical
frames, every ray at full length), fp32 and then f16, views C0, C1 and S.  For
each cap (none, 7 .. 3) method 10 and method 13 alternate twice, 2 warm-up + 10
timed frames each; m13_over_m10 is the ratio of the smaller means.  One JSON line
per cap, written to --out (default profiles/crossing/occupancy_caps.jsonl).

  python tools/crossing_caps.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossing",
                                                  "occupancy_caps.jsonl"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import bench
    from bench_crossing import frames
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n, nb, W, H = bench.CONFIGS["1024x8"]
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    pkg.synthesize((n, n, n), nb, bench.SEED)
    pkg.set_crossing_weights(np.zeros(nb, np.float32))
    pkg.set_bin_weights(np.zeros(nb, np.float32))
    for dtype in ("f32", "f16"):
        if dtype == "f16":
            pkg.convert_f16()
        for view in ("C0", "C1", "S"):
            m = bench.camera_matrix(pkg, view)
            for cap in (None, 7, 6, 5, 4, 3):
                pkg.clear_tuning()
                if cap:
                    pkg.set_tuning("VR_WG_PER_CU", str(cap))
                rec = {"tool": "crossing_caps", "dtype": dtype, "view": view, "wg_per_cu": cap}
                for _ in range(2):  # m10, m13, m10, m13
                    for method in (10, 13):
                        d = pkg.make_desc(out, W, H, m, query_method=method,
                                          volume_size=(n, n, n))
                        r = frames(pkg, torch, d, 2, 10)
                        rec.setdefault(f"m{method}_ms", []).append(r["mean_ms"])
                rec["m13_over_m10"] = round(min(rec["m13_ms"]) / min(rec["m10_ms"]), 4)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
                print(json.dumps(rec), flush=True)
    pkg.clear_tuning()
    pkg.set_crossing_weights(None)
    pkg.set_bin_weights(None)
    pkg.freeCudaBuffers()


if __name__ == "__main__":
    main()
