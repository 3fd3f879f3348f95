#!/usr/bin/env python3
"""The quantile query (method 11) against the mean (1), the entropy (3) and the
weighted-bin query (10) on one scene, in one process (tooling; DESIGN.md
section 17).

Synthesizes the config's float32 volume and, for each view, times N frames of
methods 1, 3, 10 (the CDF at 0.5: the range weights of [0, 0.5)) and 11 (the
median, q = 0.5) with HIP events (one event pair per frame after the warm-up, as
bench.py does); at the row-aligned view also the spread (0.25, 0.75).  Times
vr_bake_weighted and vr_bake_quantile (host clock around the synchronous calls)
beside vr_stream_read of the same records; times the baked method-1, method-10
and method-11 frames, all on x-row planes of the same layout; converts the volume
to f16 on the device and does all of it again.  Every frame is also rendered
once with d_steps, untimed, for its samples (the methods end rays after
different numbers of samples), so times are reported per frame and per sample.

One JSON line per measurement, appended to --out (default
profiles/quantile/bench_<config>.jsonl).

  python tools/bench_quantile.py --config 1024x8 [--views C0 C1 S] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = 0.5
SPREAD = (0.25, 0.75)


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
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f16"], choices=["f32", "f16"])
    ap.add_argument("--steps", type=int, default=20, help="timed frames per measurement")
    # two untimed frames: the first records the tile costs of the adaptive frame
    # order, the second re-deals the tiles by them (a host synchronisation)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bake-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", "quantile",
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
    base = {"tool": "bench_quantile", "config": args.config, "image": [W, H],
            "steps": args.steps, "warmup": args.warmup, "q": Q, "spread": list(SPREAD)}

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

    def ratio(a, b):
        return round(a["ns_per_sample"] / b["ns_per_sample"], 4)

    pkg.synthesize((n, n, n), nb, bench.SEED)
    pkg.set_query_range(0.0, Q, nb)  # method 10: the CDF at Q
    pkg.set_quantile(Q)
    for dtype in ("f32", "f16"):
        if dtype == "f16":
            pkg.convert_f16()
        if dtype not in args.dtypes:
            continue
        assert pkg.volume_dtype() == dtype
        pkg.set_layout_budget(None)
        # per-step frames: the parent's kernels of methods 1, 3 and 10 (1 and 3
        # with their layout copies) against k_march_quant on the x rows
        for view in args.views:
            r = {meth: measure("per_step", dtype, view, meth)
                 for meth in (1, 3, pkg.QUERY_WEIGHTED, pkg.QUERY_QUANTILE)}
            q = r[pkg.QUERY_QUANTILE]
            rec = {"what": "per_step_ratio", "dtype": dtype, "view": view,
                   "sample_m11_over_m1": ratio(q, r[1]), "sample_m11_over_m3": ratio(q, r[3]),
                   "sample_m11_over_m10": ratio(q, r[pkg.QUERY_WEIGHTED]),
                   "frame_m11_over_m1": round(q["mean_ms"] / r[1]["mean_ms"], 4)}
            if view == "C0":  # the spread against the single quantile
                pkg.set_quantile_spread(*SPREAD)
                s = measure("per_step_spread", dtype, view, pkg.QUERY_QUANTILE)
                pkg.set_quantile(Q)
                rec["sample_spread_over_single"] = ratio(s, q)
            emit(rec)
        pkg.release_stats()  # (with the layout copies of the records)
        # the bakes, against one streaming read of the same records
        rec_bytes, read_min, read_mean = pkg.stream_read(5)
        weighted_ms, quantile_ms, spread_ms = [], [], []
        for _ in range(max(args.bake_reps, 1)):
            pkg.release_weighted()
            weighted_ms.append(timed_call(pkg.bake_weighted))
            pkg.release_quantile()
            quantile_ms.append(timed_call(pkg.bake_quantile))
        pkg.set_quantile_spread(*SPREAD)
        for _ in range(max(args.bake_reps, 1)):
            pkg.release_quantile()
            spread_ms.append(timed_call(pkg.bake_quantile))
        pkg.set_quantile(Q)
        emit({"what": "bake", "dtype": dtype, "record_bytes": rec_bytes,
              "stream_read_min_ms": round(read_min, 4),
              "stream_read_gbs": round(rec_bytes / (read_min * 1e-3) / 1e9, 1),
              "bake_weighted_ms": [round(x, 3) for x in weighted_ms],
              "bake_quantile_ms": [round(x, 3) for x in quantile_ms],
              "bake_spread_ms": [round(x, 3) for x in spread_ms],
              "bake_weighted_gbs": round(rec_bytes / (min(weighted_ms) * 1e-3) / 1e9, 1),
              "bake_quantile_gbs": round(rec_bytes / (min(quantile_ms) * 1e-3) / 1e9, 1),
              "quantile_over_weighted": round(min(quantile_ms) / min(weighted_ms), 4),
              "quantile_over_stream_read": round(min(quantile_ms) / read_min, 4)})
        # baked frames: the same plane march on three planes of the same layout
        # (layout copies of the method-1 plane off); the median's rays take about
        # the mean's samples, the CDF's half as many again
        pkg.bake_quantile()
        pkg.bake_stats()
        pkg.set_layout_budget(0)
        for view in args.views:
            c = measure("baked", dtype, view, 1)
            a = measure("baked", dtype, view, pkg.QUERY_WEIGHTED)
            b = measure("baked", dtype, view, pkg.QUERY_QUANTILE)
            emit({"what": "baked_ratio", "dtype": dtype, "view": view,
                  "sample_m11_over_m10": ratio(b, a), "sample_m11_over_m1": ratio(b, c),
                  "frame_m11_over_m10": round(b["mean_ms"] / a["mean_ms"], 4),
                  "frame_m11_over_m1": round(b["mean_ms"] / c["mean_ms"], 4)})
        pkg.release_stats()
    pkg.freeCudaBuffers()


if __name__ == "__main__":
    main()
