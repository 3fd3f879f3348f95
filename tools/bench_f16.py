#!/usr/bin/env python3
"""fp32 against f16 records on one scene, one process, one JSON line (tooling).

Synthesizes the config's float32 volume, times N frames with HIP events (one
event pair per frame after the warm-up, as bench.py does), converts the
resident volume to f16 on the device (convert_f16) and times the same frames
again.  Reports both times, both kernels, both algorithmic byte counts
(footprint_bytes) and how many RGBA8 pixels the f16 frame moves.

  python tools/bench_f16.py --config 1024x8 --camera C0 --method 1 [--steps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak


def timed(pkg, torch, desc, out, warmup, steps):
    """mean / median / min ms per frame, the kernel, the frame"""
    ev = []
    for f in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pkg.render(desc)
        e1.record()
        if f >= warmup:
            ev.append((e0, e1))
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return ({"mean_ms": round(float(ms.mean()), 4), "median_ms": round(float(np.median(ms)), 4),
             "min_ms": round(float(ms.min()), 4), "kernel": pkg.last_kernel()},
            out.cpu().numpy().view(np.uint32).copy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1024x8", choices=["1024x8", "512x8", "1024x32"])
    ap.add_argument("--camera", default="C0", choices=["C0", "C1", "S"])
    ap.add_argument("--method", type=int, default=1, choices=[1, 2, 3])
    ap.add_argument("--steps", type=int, default=20, help="timed frames per volume (>= 20)")
    # two untimed frames: the first records the tile costs of the adaptive frame
    # order, the second re-deals the tiles by them (a host synchronisation)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tuning", nargs="*", default=[], metavar="KEY=VALUE",
                    help="vr_set_tuning knobs for the f16 frames only, e.g. VR_WG_PER_CU=3")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be >= 20")
    import torch
    import __graft_entry__ as g
    import bench
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n, nb, W, H = bench.CONFIGS[args.config]
    m = bench.camera_matrix(pkg, args.camera)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    desc = pkg.make_desc(out, W, H, m, query_method=args.method, volume_size=(n, n, n))
    pkg.synthesize((n, n, n), nb, bench.SEED)
    res = {"tool": "bench_f16", "config": args.config, "camera": args.camera,
           "method": args.method, "image": [W, H], "steps": args.steps, "warmup": args.warmup,
           "f16_tuning": args.tuning, "lib": os.path.relpath(pkg.LIB_PATH, ROOT)}
    frames = {}
    for dt in ("f32", "f16"):
        if dt == "f16":
            pkg.convert_f16()
            out.zero_()
            for kv in args.tuning:
                pkg.set_tuning(*kv.split("=", 1))
        assert pkg.volume_dtype() == dt
        r, frames[dt] = timed(pkg, torch, desc, out, max(args.warmup, 1), args.steps)
        r["footprint_bytes"] = int(pkg.footprint_bytes(desc))
        r["frac_hbm_peak"] = round(r["footprint_bytes"] / (r["mean_ms"] * 1e-3) / 1e9
                                   / HBM_PEAK_GBS, 4)
        res[dt] = r
    res["f16_over_f32"] = round(res["f16"]["mean_ms"] / res["f32"]["mean_ms"], 4)
    res["rgba8_mismatch"] = int(np.sum(frames["f32"] != frames["f16"]))
    res["hit_pixels"] = int(np.sum(frames["f32"] != 0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
