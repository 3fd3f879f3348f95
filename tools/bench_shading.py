#!/usr/bin/env python3
"""What the headlight costs against the existing table march over the same samples,
in one process (tooling).

Synthesizes the config's volume, narrows it to f16, bakes the method-10 plane of the
range [0, 0.3) and the method-13 plane of the isovalue 0.3, and for each view and each
of two tables times N frames of

  the yardstick   the existing k_march_plane_tf frame of the plane under the table, and
  matte, shiny    the k_march_lit frame of the same plane under the same table and the
                  default light (0.3, 0.7, 0, shininess 1: no highlight is computed)
                  or the light (0.2, 0.5, 0.6, shininess 16),

with HIP events (one event pair per frame after the warm-up, as bench.py does).  The
tables: `rand`, 256 random entries (rays end early by opacity), and `clear`, the same
with alpha 0 (every ray runs to its end: the most samples per frame).  Every frame is
rendered once more with d_steps, untimed, and the tool asserts that the lit frame's
samples per pixel equal the yardstick's: the same rays, the same steps, the same
loads, so the ratio is that of the arithmetic alone.

One JSON line per measurement, appended to --out.

  python tools/bench_shading.py --config 1024x8 [--views C0 C1 S] [--steps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THETA = 0.3
LIGHTS = {"matte": dict(ambient=0.3, diffuse=0.7, specular=0.0, shininess=1),
          "shiny": dict(ambient=0.2, diffuse=0.5, specular=0.6, shininess=16)}


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
    out_path = args.out or os.path.join(ROOT, "profiles", "shading", f"bench_{args.config}.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    import torch
    import __graft_entry__ as g
    import bench
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n, nb, W, H = bench.CONFIGS[args.config]
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    steps_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    base = {"tool": "bench_shading", "config": args.config, "image": [W, H], "dtype": "f16",
            "steps": args.steps, "warmup": args.warmup}
    rand = np.random.default_rng(1401).random((256, 4)).astype(np.float32)
    clear = rand.copy()
    clear[:, 3] = 0  # transparent everywhere
    tables = {"rand": rand, "clear": clear}

    def emit(rec):
        rec = dict(base, **rec)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    def measure(what, view, method, table, light):
        pkg.set_light(**light) if light else pkg.set_light(None)
        m = bench.camera_matrix(pkg, view)
        desc = pkg.make_desc(out, W, H, m, query_method=method, volume_size=(n, n, n))
        r = frames(pkg, torch, desc, max(args.warmup, 1), args.steps)
        pkg.render(pkg.make_desc(out, W, H, m, query_method=method, volume_size=(n, n, n),
                                 d_steps=steps_buf))
        torch.cuda.synchronize()
        s = steps_buf.cpu().numpy().copy()
        r["samples"] = int(s[s > 0].sum())
        r["rays"] = int((s >= 0).sum())
        r["ns_per_sample"] = round(r["mean_ms"] * 1e6 / max(r["samples"], 1), 5)
        emit(dict(r, what=what, view=view, method=method, table=table))
        return r, s

    pkg.synthesize((n, n, n), nb, bench.SEED)
    pkg.convert_f16()
    pkg.set_query_range(0.0, THETA, nb)
    pkg.set_isovalue(THETA, nb)
    pkg.bake_weighted()
    pkg.bake_crossing()
    try:
        for method in (pkg.QUERY_WEIGHTED, pkg.QUERY_CROSSING):
            for name, table in tables.items():
                pkg.set_transfer_function(table)
                for view in args.views:
                    a, sa = measure("yardstick", view, method, name, None)
                    assert "k_march_plane_tf" in a["kernel"], a["kernel"]
                    for lname, light in LIGHTS.items():
                        b, sb = measure(lname, view, method, name, light)
                        assert "k_march_lit" in b["kernel"], b["kernel"]
                        assert np.array_equal(sa, sb), \
                            f"method {method} {view} {name} {lname}: d_steps differ"
                        emit({"what": "ratio", "light": lname, "view": view, "method": method,
                              "table": name, "lit_kernel": b["kernel"],
                              "yardstick_kernel": a["kernel"], "lit_ms": b["mean_ms"],
                              "yardstick_ms": a["mean_ms"],
                              "frame_lit_over_yardstick": round(b["mean_ms"] / a["mean_ms"], 4),
                              "frame_min_lit_over_yardstick": round(b["min_ms"] / a["min_ms"], 4),
                              "samples": a["samples"], "same_steps": True})
    finally:
        pkg.set_light(None)
        pkg.set_transfer_function(None)
        pkg.set_crossing_weights(None)
        pkg.set_bin_weights(None)
        pkg.freeCudaBuffers()


if __name__ == "__main__":
    main()
