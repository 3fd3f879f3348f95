#!/usr/bin/env python3
"""What a gradient-magnitude plane costs to bake and to render, in one process
(tooling).

Synthesizes the config's volume, narrows it to f16, bakes the statistics planes
(method 1: the mean; 2: the variance) and the method-13 plane of the isovalue 0.3.

  bake     wall-clock ms of bake_gradient(1) and bake_gradient(13), each baked
           --bakes times (released in between; the first is reported apart), the whole
           synchronous call: two allocations, the clearing of the plane, k_bake_grad,
           the read-back of the maximum.  The yardstick is the existing plane-to-plane
           copy k_plane8 of the same mean plane: layout_info()["last_build_ms"] after
           a baked C1 frame of method 1, which times the copy's clearing, its kernel
           and the synchronise.
  frames   for each view N frames with HIP events (one event pair per frame after the
           warm-up, as bench.py does) of the mean / |grad mean| pair under a seeded
           32 x 32 table (v_scale = 1 / max), against the mean / variance pair under
           the same table: k_march_tf2 both times, the same u plane, so the same rays
           set out; they end where the table's opacity along v ends them, so samples
           and ns per sample are reported beside the frame times.

One JSON line per measurement, appended to --out.

  python tools/bench_gradient.py --config 1024x8 [--views C0 C1 S] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THETA = 0.3


def frames(pkg, torch, desc, warmup, steps):
    """mean / median / min ms per frame and the kernel that rendered them"""
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
    return {"mean_ms": round(float(ms.mean()), 4), "median_ms": round(float(np.median(ms)), 4),
            "min_ms": round(float(ms.min()), 4), "kernel": pkg.last_kernel()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1024x8",
                    choices=["256x4", "512x8", "1024x8", "512x32", "1024x16", "1024x32"])
    ap.add_argument("--views", nargs="+", default=["C0", "C1", "S"], choices=["C0", "C1", "S"])
    ap.add_argument("--steps", type=int, default=20, help="timed frames per measurement")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bakes", type=int, default=5, help="bakes per source")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", "gradient", f"bench_{args.config}.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    import torch
    import __graft_entry__ as g
    import bench
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n, nb, W, H = bench.CONFIGS[args.config]
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    steps_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    base = {"tool": "bench_gradient", "config": args.config, "image": [W, H], "dtype": "f16",
            "steps": args.steps, "warmup": args.warmup}
    rand32 = np.random.default_rng(1701).random((32, 32, 4)).astype(np.float32)

    def emit(rec):
        rec = dict(base, **rec)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    def measure(what, view, method, set_table):
        set_table()
        m = bench.camera_matrix(pkg, view)
        desc = pkg.make_desc(out, W, H, m, query_method=method, volume_size=(n, n, n))
        r = frames(pkg, torch, desc, max(args.warmup, 1), args.steps)
        pkg.render(pkg.make_desc(out, W, H, m, query_method=method, volume_size=(n, n, n),
                                 d_steps=steps_buf))
        torch.cuda.synchronize()
        s = steps_buf.cpu().numpy()
        r["samples"] = int(s[s > 0].sum())
        r["rays"] = int((s >= 0).sum())
        r["ns_per_sample"] = round(r["mean_ms"] * 1e6 / max(r["samples"], 1), 5)
        emit(dict(r, what=what, view=view, method=method))
        return r

    pkg.synthesize((n, n, n), nb, bench.SEED)
    pkg.convert_f16()
    # the stream-read ceiling as bench.py --full reports it: the records read once
    rb, rms, _ = pkg.stream_read(8)
    emit({"what": "read_ceiling", "kernel": "k_stream_read", "bytes": rb, "ms": round(rms, 4),
          "GBps": round(rb / (rms * 1e-3) / 1e9, 1)})
    pkg.set_isovalue(THETA, nb)
    pkg.bake_stats()
    pkg.bake_crossing()
    try:
        # the yardstick: the 8 x 2 x 2 brick copy of the mean plane a baked C1 frame makes
        builds = pkg.layout_info()["builds"]
        pkg.render(pkg.make_desc(out, W, H, bench.camera_matrix(pkg, "C1"), query_method=1,
                                 volume_size=(n, n, n)))
        torch.cuda.synchronize()
        info = pkg.layout_info()
        if info["builds"] == builds + 1:
            emit({"what": "plane8_copy", "ms": info["last_build_ms"],
                  "bytes": info["last_build_bytes"], "kernel": pkg.last_kernel()})
        else:
            emit({"what": "plane8_copy", "ms": None, "note": "the C1 frame made no layout copy"})
        pkg.release_stats()  # (with the copy; the planes again, without it)
        pkg.bake_stats()
        pkg.set_isovalue(THETA, nb)
        pkg.bake_crossing()
        voxels = n ** 3
        for src in (1, 13):
            ms = []
            for _ in range(args.bakes):
                pkg.release_gradient(src)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pkg.bake_gradient(src)
                ms.append((time.perf_counter() - t0) * 1e3)
            ptr, floats, mx = pkg.gradient_info(src)
            rest = np.array(ms[1:] or ms)
            emit({"what": "bake_gradient", "source": src, "first_ms": round(ms[0], 3),
                  "mean_ms": round(float(rest.mean()), 3), "min_ms": round(float(rest.min()), 3),
                  "plane_bytes": 4 * floats, "max": mx,
                  "gb_per_s_4in_4out": round(8e-6 * voxels / float(rest.min()), 1)})
        mx = pkg.gradient_info(1)[2]
        for view in args.views:
            a = measure("tf2_mean_variance", view, 1,
                        lambda: pkg.set_transfer_function_2d(rand32, 2, 0.0, 3.0))
            b = measure("tf2_mean_gradient", view, 1, lambda: pkg.set_transfer_function_2d(
                rand32, pkg.gradient_of(1), 0.0, 1.0 / mx))
            assert "k_march_tf2" in a["kernel"] and a["kernel"] == b["kernel"]
            emit({"what": "ratio_pair", "view": view, "kernel": b["kernel"],
                  "gradient_ms": b["mean_ms"], "variance_ms": a["mean_ms"],
                  "frame_gradient_over_variance": round(b["mean_ms"] / a["mean_ms"], 4),
                  "frame_min_gradient_over_variance": round(b["min_ms"] / a["min_ms"], 4),
                  "gradient_samples": b["samples"], "variance_samples": a["samples"],
                  "gradient_ns_per_sample": b["ns_per_sample"],
                  "variance_ns_per_sample": a["ns_per_sample"]})
    finally:
        pkg.set_transfer_function_2d(None)
        pkg.set_crossing_weights(None)
        pkg.freeCudaBuffers()


if __name__ == "__main__":
    main()
