#!/usr/bin/env python3
"""What a user-defined transfer function costs a baked frame, in one process
(tooling).

Synthesizes the config's volume, narrows it to f16, bakes the method-10 plane of
the range [0, 0.3) and the method-13 plane of the isovalue 0.3, and for each view
times N frames of the plane with no table set -- the existing plane march: the
plan's kernel for method 10, k_march_cross_plane for method 13 -- and N frames of
the same plane with the reference's nine entries set as a custom table
(k_march_plane_tf), with HIP events (one event pair per frame after the warm-up, as
bench.py does).  The two frames must be identical, and the tool asserts it: the same
rays, the same samples, the same early exits, so the ratio is the cost of the new
kernel alone.  For method 13 both kernels are the same one-lane march, so that ratio
isolates the LDS lookup; for method 10 at oblique views the existing frame is the
four-lane k_march_seg4, and the ratio holds that gap as well.  One line per plane
and view with a seeded random 256-entry table follows, for information (its rays
end elsewhere).  Every frame is rendered once more with d_steps, untimed, for its
samples.

One JSON line per measurement, appended to --out.

  python tools/bench_transfer.py --config 1024x8 [--views C0 C1 S] [--steps 20]
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
    out_path = args.out or os.path.join(ROOT, "profiles", "transfer",
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
    base = {"tool": "bench_transfer", "config": args.config, "image": [W, H], "dtype": "f16",
            "steps": args.steps, "warmup": args.warmup}
    rand256 = np.random.default_rng(1401).random((256, 4)).astype(np.float32)

    def emit(rec):
        rec = dict(base, **rec)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    def measure(what, view, method, table):
        pkg.set_transfer_function(table)
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
    pkg.set_query_range(0.0, THETA, nb)
    pkg.set_isovalue(THETA, nb)
    pkg.bake_weighted()
    pkg.bake_crossing()
    try:
        for method in (pkg.QUERY_WEIGHTED, pkg.QUERY_CROSSING):
            for view in args.views:
                a, fa = measure("built_in", view, method, None)
                b, fb = measure("reference_tf", view, method, pkg.REFERENCE_TF)
                assert "k_march_plane_tf" in b["kernel"] and "plane_tf" not in a["kernel"]
                assert np.array_equal(fa, fb), f"method {method} {view}: the frames differ"
                assert a["samples"] == b["samples"]
                emit({"what": "ratio", "view": view, "method": method,
                      "tf_kernel": b["kernel"], "built_in_kernel": a["kernel"],
                      "tf_ms": b["mean_ms"], "built_in_ms": a["mean_ms"],
                      "frame_tf_over_built_in": round(b["mean_ms"] / a["mean_ms"], 4),
                      "frame_min_tf_over_built_in": round(b["min_ms"] / a["min_ms"], 4),
                      "samples": a["samples"], "same_frame": True})
                measure("rand256", view, method, rand256)
    finally:
        pkg.set_transfer_function(None)
        pkg.set_crossing_weights(None)
        pkg.set_bin_weights(None)
        pkg.freeCudaBuffers()


if __name__ == "__main__":
    main()
