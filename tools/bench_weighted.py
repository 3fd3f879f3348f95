#!/usr/bin/env python3
"""The weighted-bin query (method 10) against the mean (method 1) on one scene, in
one process (tooling).

Synthesizes the config's float32 volume and, for each view, times N frames of
method 1 and of method 10 (the range probability P(0.25 <= v < 0.75), and the
weights (i + 1/2) / B that make it the normalised mean, whose rays take method
1's samples) with HIP events (one event pair per frame after the warm-up, as
bench.py does); times
vr_bake_stats and vr_bake_weighted (host clock around the synchronous calls)
beside vr_stream_read of the same records; times the baked method-1 and
method-10 frames with layout copies off; converts the volume to f16 on the
device and does all of it again.  Every frame is also rendered once with
d_steps, untimed, for its samples (the two methods end rays after different
numbers of samples), so times are reported per frame and per sample.

One JSON line per measurement, appended to --out (default
profiles/weighted/bench_<config>.jsonl).

  python tools/bench_weighted.py --config 1024x8 [--views C0 C1 S] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LO, HI = 0.25, 0.75


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
    # two untimed frames: the first records the tile costs of the adaptive frame
    # order, the second re-deals the tiles by them (a host synchronisation)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bake-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", "weighted",
                                        f"bench_{args.config}.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    import torch
    import __graft_entry__ as g
    import bench
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n, nb, W, H = bench.CONFIGS[args.config]
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    steps_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    base = {"tool": "bench_weighted", "config": args.config, "image": [W, H],
            "steps": args.steps, "warmup": args.warmup, "range": [LO, HI]}

    def emit(rec):
        rec = dict(base, **rec)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    def measure(what, dtype, view, method):
        m = bench.camera_matrix(pkg, view)
        desc = pkg.make_desc(out, W, H, m, query_method=method, volume_size=(n, n, n))
        r = frames(pkg, torch, desc, max(args.warmup, 1), args.steps)
        # the same frame once more with d_steps, untimed: its samples
        pkg.render(pkg.make_desc(out, W, H, m, query_method=method, volume_size=(n, n, n),
                                 d_steps=steps_buf))
        torch.cuda.synchronize()
        s = steps_buf.cpu().numpy()
        r["samples"] = int(s[s > 0].sum())
        r["rays"] = int((s >= 0).sum())
        r["ns_per_sample"] = round(r["mean_ms"] * 1e6 / max(r["samples"], 1), 5)
        emit(dict(r, what=what, dtype=dtype, view=view, method=method))
        return r

    def timed_call(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    pkg.synthesize((n, n, n), nb, bench.SEED)
    pkg.set_query_range(LO, HI, nb)
    # like for like: w_i = (i + 1/2) / B makes method 10 the normalised mean up to
    # rounding, so its rays take (nearly) method 1's samples and read its records
    mean_w = ((np.arange(nb, dtype=np.float64) + 0.5) / nb).astype(np.float32)
    for dtype in ("f32", "f16"):
        if dtype == "f16":
            pkg.convert_f16()
        assert pkg.volume_dtype() == dtype
        pkg.set_layout_budget(None)
        # per-step frames: the parent's method-1 kernels (with their layout
        # copies) against k_march_lin on the x rows
        for view in args.views:
            a = measure("per_step", dtype, view, 1)
            b = measure("per_step", dtype, view, pkg.QUERY_WEIGHTED)
            pkg.set_bin_weights(mean_w)
            c = measure("per_step_meanw", dtype, view, pkg.QUERY_WEIGHTED)
            pkg.set_query_range(LO, HI, nb)
            emit({"what": "per_step_ratio", "dtype": dtype, "view": view,
                  "frame_m10_over_m1": round(b["mean_ms"] / a["mean_ms"], 4),
                  "sample_m10_over_m1": round(b["ns_per_sample"] / a["ns_per_sample"], 4),
                  "frame_meanw_over_m1": round(c["mean_ms"] / a["mean_ms"], 4),
                  "sample_meanw_over_m1": round(c["ns_per_sample"] / a["ns_per_sample"], 4)})
        pkg.release_stats()  # (with the layout copies of the records)
        # the bakes, against one streaming read of the same records
        rec_bytes, read_min, read_mean = pkg.stream_read(5)
        stats_ms, weighted_ms = [], []
        for _ in range(max(args.bake_reps, 1)):
            pkg.release_stats()
            stats_ms.append(timed_call(pkg.bake_stats))
            pkg.release_weighted()
            weighted_ms.append(timed_call(pkg.bake_weighted))
        emit({"what": "bake", "dtype": dtype, "record_bytes": rec_bytes,
              "stream_read_min_ms": round(read_min, 4),
              "stream_read_gbs": round(rec_bytes / (read_min * 1e-3) / 1e9, 1),
              "bake_stats_ms": [round(x, 3) for x in stats_ms],
              "bake_weighted_ms": [round(x, 3) for x in weighted_ms],
              "bake_stats_gbs": round(rec_bytes / (min(stats_ms) * 1e-3) / 1e9, 1),
              "bake_weighted_gbs": round(rec_bytes / (min(weighted_ms) * 1e-3) / 1e9, 1),
              "weighted_over_stats": round(min(weighted_ms) / min(stats_ms), 4)})
        # baked frames, both on x-row planes of the same layout (no plane copies)
        pkg.set_layout_budget(0)
        base_m1, base_m10 = {}, {}
        for view in args.views:
            base_m1[view] = measure("baked", dtype, view, 1)
            base_m10[view] = measure("baked", dtype, view, pkg.QUERY_WEIGHTED)
        pkg.set_bin_weights(mean_w)  # (drops the plane of the range weights)
        pkg.bake_weighted()
        for view in args.views:
            a, b = base_m1[view], base_m10[view]
            c = measure("baked_meanw", dtype, view, pkg.QUERY_WEIGHTED)
            emit({"what": "baked_ratio", "dtype": dtype, "view": view,
                  "frame_m10_over_m1": round(b["mean_ms"] / a["mean_ms"], 4),
                  "sample_m10_over_m1": round(b["ns_per_sample"] / a["ns_per_sample"], 4),
                  "frame_meanw_over_m1": round(c["mean_ms"] / a["mean_ms"], 4),
                  "sample_meanw_over_m1": round(c["ns_per_sample"] / a["ns_per_sample"], 4)})
        pkg.set_query_range(LO, HI, nb)
        pkg.release_stats()
    pkg.freeCudaBuffers()


if __name__ == "__main__":
    main()
