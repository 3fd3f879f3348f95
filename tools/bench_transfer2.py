#!/usr/bin/env python3
"""What a 2-D transfer function over two planes costs a baked frame, in one process
(tooling).

Synthesizes the config's volume, narrows it to f16, bakes the statistics planes
(method 1: the mean) and the method-13 plane of the isovalue 0.3, and for each view
times N frames with HIP events (one event pair per frame after the warm-up, as
bench.py does).  Every bar is stated against frames measured in the same process:

  (a) the lookup's cost.  An 8-bit 1-D table is set (k_march_plane_tf on the
      method-13 plane), then the same table repeated over nv = 4 with u = v = 13
      (k_march_tf2).  The two frames must be identical, and the tool asserts it: the
      same rays, the same samples, the same early exits, so the ratio isolates the
      second gather -- which hits the same lines -- and the two extra LDS reads.
  (b) the real case.  u = 1 (mean), v = 13 with a seeded random 32 x 32 table,
      against the sum of the two one-plane frames under that table's row 0, u alone
      and v alone (k_march_plane_tf), measured back to back.  The two-plane frame
      does at most their combined gathers in one march; its rays end elsewhere, so
      ns per sample is reported beside the frame times.

Every frame is rendered once more with d_steps, untimed, for its samples.  One JSON
line per measurement, appended to --out.

  python tools/bench_transfer2.py --config 1024x8 [--views C0 C1 S] [--steps 20]
"""
import argparse
import json
import os
import sys

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
    # two untimed frames: the first records the tile costs of the adaptive frame
    # order, the second re-deals the tiles by them (a host synchronisation)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", "transfer2",
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
    base = {"tool": "bench_transfer2", "config": args.config, "image": [W, H], "dtype": "f16",
            "steps": args.steps, "warmup": args.warmup}
    rng = np.random.default_rng(1601)
    tab8 = rng.integers(0, 257, (256, 4)).astype(np.float32) / np.float32(256)
    rand32 = rng.random((32, 32, 4)).astype(np.float32)

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
        frame = out.cpu().numpy().copy()
        pkg.render(pkg.make_desc(out, W, H, m, query_method=method, volume_size=(n, n, n),
                                 d_steps=steps_buf))
        torch.cuda.synchronize()
        s = steps_buf.cpu().numpy()
        r["samples"] = int(s[s > 0].sum())
        r["rays"] = int((s >= 0).sum())
        r["ns_per_sample"] = round(r["mean_ms"] * 1e6 / max(r["samples"], 1), 5)
        emit(dict(r, what=what, view=view, method=method))
        return r, frame

    pkg.synthesize((n, n, n), nb, bench.SEED)
    pkg.convert_f16()
    pkg.set_isovalue(THETA, nb)
    pkg.bake_stats()
    pkg.bake_crossing()
    try:
        for view in args.views:
            # (a) the lookup: the same frame through both kernels
            a, fa = measure("tf1_8bit", view, 13, lambda: pkg.set_transfer_function(tab8))
            b, fb = measure("tf2_rows_of_tf1", view, 13, lambda: pkg.set_transfer_function_2d(
                np.repeat(tab8[None], 4, axis=0), 13))
            assert "k_march_plane_tf" in a["kernel"] and "k_march_tf2" in b["kernel"]
            assert np.array_equal(fa, fb), f"{view}: the 1-D and the 2-D frame differ"
            assert a["samples"] == b["samples"]
            emit({"what": "ratio_lookup", "view": view, "tf2_kernel": b["kernel"],
                  "tf1_kernel": a["kernel"], "tf2_ms": b["mean_ms"], "tf1_ms": a["mean_ms"],
                  "frame_tf2_over_tf1": round(b["mean_ms"] / a["mean_ms"], 4),
                  "frame_min_tf2_over_tf1": round(b["min_ms"] / a["min_ms"], 4),
                  "samples": a["samples"], "same_frame": True})
            # (b) colour by the mean, opacity by the crossing probability
            row0 = rand32[0]
            u, _ = measure("tf1_row0_u", view, 1, lambda: pkg.set_transfer_function(row0))
            v, _ = measure("tf1_row0_v", view, 13, lambda: pkg.set_transfer_function(row0))
            t, _ = measure("tf2_rand32", view, 1,
                           lambda: pkg.set_transfer_function_2d(rand32, 13))
            assert "k_march_tf2" in t["kernel"]
            both = u["mean_ms"] + v["mean_ms"]
            emit({"what": "ratio_pair", "view": view, "tf2_kernel": t["kernel"],
                  "tf2_ms": t["mean_ms"], "u_ms": u["mean_ms"], "v_ms": v["mean_ms"],
                  "sum_ms": round(both, 4), "frame_tf2_over_sum": round(t["mean_ms"] / both, 4),
                  "tf2_samples": t["samples"], "u_samples": u["samples"],
                  "v_samples": v["samples"], "tf2_ns_per_sample": t["ns_per_sample"],
                  "sum_ns_per_sample": round(u["ns_per_sample"] + v["ns_per_sample"], 5)})
    finally:
        pkg.set_transfer_function(None)
        pkg.set_transfer_function_2d(None)
        pkg.set_crossing_weights(None)
        pkg.freeCudaBuffers()


if __name__ == "__main__":
    main()
