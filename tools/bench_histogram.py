#!/usr/bin/env python3
"""What a value range and a histogram of resident baked planes cost, in one process
(tooling).

Synthesizes the config's volume, narrows it to f16, bakes the statistics planes (method
1: the mean), the gradient plane of the mean, and a constant plane: the weighted-bin
plane (method 10) of weights that are all 0, which is +0 at every voxel, with its
gradient plane, +0 as well.

  range      plane_range of the mean plane
  hist       plane_histogram of the mean plane over 256 bins, and of the mean /
             gradient_of(1) pair over 64 x 64 and 128 x 128 bins, windows from
             plane_window
  constant   the same three histograms of the constant plane(s): every voxel in one
             bin, the contention worst case

For each, --reps calls after one warm-up: the kernel's time by HIP events
(plane_kernel_ms: the events are recorded on the library's stream around the one
kernel) and the wall clock of the whole synchronous call (allocation, clearing,
kernel, read-back).  The yardstick is stream_read's measured read ceiling of the same
process applied to the bytes of the plane buffers the kernel reads: stream_ms =
plane bytes / ceiling, and ratio = kernel ms / stream_ms.

One JSON line per measurement, appended to --out.

  python tools/bench_histogram.py --config 1024x8 [--reps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1024x8",
                    choices=["256x4", "512x8", "1024x8", "512x32", "1024x16", "1024x32"])
    ap.add_argument("--reps", type=int, default=10, help="timed calls per measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", "histogram", f"bench_{args.config}.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    import torch
    import __graft_entry__ as g
    import bench
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n, nb, _, _ = bench.CONFIGS[args.config]
    base = {"tool": "bench_histogram", "config": args.config, "dtype": "f16", "reps": args.reps}

    def emit(rec):
        rec = dict(base, **rec)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    pkg.synthesize((n, n, n), nb, bench.SEED)
    pkg.convert_f16()
    rb, rms, rmean = pkg.stream_read(8)
    ceiling = rb / (rms * 1e-3)  # bytes per second, the fastest pass
    emit({"what": "read_ceiling", "kernel": "k_stream_read", "bytes": rb, "ms": round(rms, 4),
          "mean_ms": round(rmean, 4), "GBps": round(ceiling / 1e9, 1)})
    voxels = n ** 3
    try:
        pkg.bake_stats()
        pkg.bake_gradient(1)
        pkg.set_bin_weights(np.zeros(nb, np.float32))
        pkg.bake_weighted()
        pkg.bake_gradient(10)
        plane_bytes = 4 * pkg.weighted_info()[1]

        def measure(what, planes, call):
            call()  # warm-up: the code object, the first touch of the planes
            kern, wall = [], []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(pkg.plane_kernel_ms())
            kern, wall = np.array(kern), np.array(wall)
            stream_ms = planes * plane_bytes / ceiling * 1e3
            rec = {"what": what, "kernel": pkg.last_kernel(), "planes": planes,
                   "plane_bytes": plane_bytes, "kernel_ms": round(float(kern.mean()), 4),
                   "kernel_min_ms": round(float(kern.min()), 4),
                   "kernel_max_ms": round(float(kern.max()), 4),
                   "wall_ms": round(float(wall.mean()), 4), "wall_min_ms": round(float(wall.min()), 4),
                   "stream_ms": round(stream_ms, 4),
                   "ratio": round(float(kern.mean()) / stream_ms, 4),
                   "ratio_min": round(float(kern.min()) / stream_ms, 4)}
            if isinstance(res, np.ndarray):
                assert int(res.sum()) == voxels, (what, int(res.sum()))
                rec["bins_used"] = int((res > 0).sum())
                rec["largest_bin"] = int(res.max())
            else:
                rec["range"] = [float(res[0]), float(res[1]), int(res[2])]
            emit(rec)
            return rec

        g1 = pkg.gradient_of(1)
        wu, wv = pkg.plane_window(1), pkg.plane_window(g1)
        emit({"what": "windows", "mean": wu, "gradient": wv})
        measure("range_mean", 1, lambda: pkg.plane_range(1))
        synth = {
            "hist_256": measure("hist_256", 1, lambda: pkg.plane_histogram(1, 256, wu)),
            "hist_64x64": measure("hist_64x64", 2,
                                  lambda: pkg.plane_histogram(1, 64, wu, g1, 64, wv)),
            "hist_128x128": measure("hist_128x128", 2,
                                    lambda: pkg.plane_histogram(1, 128, wu, g1, 128, wv)),
        }
        # the constant planes: +0 everywhere, at the middle of the window (-0.5, 1)
        g10, wc = pkg.gradient_of(10), (-0.5, 1.0)
        assert pkg.plane_range(10)[:2] == (0.0, 0.0) and pkg.plane_range(g10)[:2] == (0.0, 0.0)
        const = {
            "hist_256": measure("constant_hist_256", 1, lambda: pkg.plane_histogram(10, 256, wc)),
            "hist_64x64": measure("constant_hist_64x64", 2,
                                  lambda: pkg.plane_histogram(10, 64, wc, g10, 64, wc)),
            "hist_128x128": measure("constant_hist_128x128", 2,
                                    lambda: pkg.plane_histogram(10, 128, wc, g10, 128, wc)),
        }
        for k in synth:
            assert const[k]["largest_bin"] == voxels
            emit({"what": "constant_over_synthetic", "case": k,
                  "ratio": round(const[k]["kernel_ms"] / synth[k]["kernel_ms"], 4)})
        for k in ("hist_256", "hist_64x64"):
            emit({"what": "bar", "case": k, "kernel_ms": synth[k]["kernel_ms"],
                  "stream_ms": synth[k]["stream_ms"], "ratio": synth[k]["ratio"], "bar": 1.25,
                  "met": bool(synth[k]["ratio"] <= 1.25)})
    finally:
        pkg.set_bin_weights(None)
        pkg.freeCudaBuffers()


if __name__ == "__main__":
    main()
