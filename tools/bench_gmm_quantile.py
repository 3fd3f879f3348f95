#!/usr/bin/env python3
"""The quantile of GMM volumes against its yardsticks, one process, JSON lines
(tooling).

Synthesizes the gmm1024 volume (1024^3 x 16, 1080p) as f16 (or --dtype f32), sets
the median (q = 0.5) and the range [0.25, 0.75) and measures, each line beside the
parent's code doing the nearest thing in the same process:

  1. per-step frames of method 11 (k_march_gmm_quant) at every camera, against
     the method-10 frame (k_march_gmm_range), which gathers the same bytes and
     reads the same table: time, samples per frame and time per sample;
  2. the quantile bake (bake_gmm_quantile) against bake_gmm_range and
     bake_gmm_stats on the same records -- for each the first bake, which also
     allocates and zeroes its planes, and --bakes re-bakes -- with GB/s of records
     read and the fraction of the vr_stream_read ceiling of this process (a
     1024^3 x 8 float32 histogram volume synthesized and released before the GMM
     volume is made; --no-ceiling skips it);
  3. the spread (0.25, 0.75) against the median at the first camera: the per-step
     frame and the bake (records still resident);
  4. with the records freed, frames from the quantile plane against frames from
     the range plane: the same plane march on the same layout, ray lengths differ
     with content, so samples per frame stand beside the times.  The baked
     method-11 frame is compared with the per-step one pixel by pixel; so is the
     baked spread frame at the first camera.

HIP events, one pair per frame after the warm-up.  Every GPU step runs under its
own time limit: a step that overruns ends the process at once (exit status 1, the
Python stacks on stderr) and nothing more is started on the GPU.

  python tools/bench_gmm_quantile.py > profiles/gmm_quantile/bench_gmm1024_f16.jsonl
  python tools/bench_gmm_quantile.py --dtype f32 > profiles/gmm_quantile/bench_gmm1024_f32.jsonl
  python tools/bench_gmm_quantile.py --config gmm96 --no-ceiling     # a quick check of the tool
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_gmm_baked import ELEM, limit, note, stats  # noqa: E402
from bench_gmm_range import timed_bakes, timed_frames  # noqa: E402

RANGE = (0.25, 0.75)
MEDIAN = 0.5
SPREAD = (0.25, 0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gmm1024", choices=["gmm1024", "gmm96"],
                    help="scene (gmm96: a quick check of the tool)")
    ap.add_argument("--dtype", default="f16", choices=["f16", "f32"])
    ap.add_argument("--cameras", default="C0,C1,S", help="comma list of C0, C1, S (side view)")
    ap.add_argument("--steps", type=int, default=20, help="timed frames per line (>= 20)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bakes", type=int, default=3, help="timed re-bakes after each first bake")
    ap.add_argument("--no-ceiling", action="store_true", help="skip the vr_stream_read ceiling")
    ap.add_argument("--step-limit", type=int, default=240,
                    help="seconds each GPU step may take before the process is ended")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be >= 20")
    cams = args.cameras.split(",")
    if not set(cams) <= {"C0", "C1", "S"}:
        ap.error("cameras are C0 / C1 / S")
    args.warmup = max(args.warmup, 1)
    import torch
    import __graft_entry__ as g
    import bench
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n, K, W, H = bench.GMM_CONFIGS[args.config]
    dt = args.dtype
    base = {"tool": "bench_gmm_quantile", "scene": args.config, "volume": [n, n, n], "K": K,
            "dtype": dt, "image": [W, H], "q": MEDIAN, "spread": list(SPREAD),
            "range": list(RANGE), "search_steps": pkg.gmm_quantile_steps(),
            "lib": os.path.relpath(pkg.LIB_PATH, ROOT)}
    s = torch.cuda.Stream()
    pkg.set_stream(s)

    ceiling = None
    if not args.no_ceiling:
        with limit(args.step_limit, "read ceiling"):
            pkg.synthesize((n, n, n), 8, bench.SEED)
            nbytes, best_ms, mean_ms = pkg.stream_read(5)
            pkg.freeCudaBuffers()
        ceiling = nbytes / (best_ms * 1e-3) / 1e9
        print(json.dumps(dict(base, kind="ceiling", bytes=nbytes, best_ms=round(best_ms, 4),
                              mean_ms=round(mean_ms, 4), GBps=round(ceiling, 1))), flush=True)

    with limit(args.step_limit, f"synthesize {dt} {n}^3 x {K}"):
        pkg.synthesize_gmm((n, n, n), K, bench.SEED, dtype=dt)
        torch.cuda.synchronize()
    pkg.set_gmm_range(*RANGE)
    pkg.set_quantile(MEDIAN)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    nsteps = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    desc = {(c, m): pkg.make_desc(out, W, H, bench.camera_matrix(pkg, c), query_method=m,
                                  volume_size=(1, 1, 1), d_steps=nsteps)
            for c in cams for m in (10, 11)}

    def frames(render, c, m, what):
        with limit(args.step_limit, f"{what} {c} m{m}"):
            r, f = timed_frames(pkg, torch, s, render, desc[c, m], out, nsteps, args.warmup,
                                args.steps)
        note(f"{what} {c} m{m}: {r['mean_ms']} ms, {r['samples']} samples  {r['kernel']}")
        return r, f

    def ratios(r, yard):
        return {"time_ratio": round(r["mean_ms"] / yard["mean_ms"], 4),
                "per_sample_ratio": round(r["ns_per_sample"] / yard["ns_per_sample"], 4)}

    per_step, median_step = {}, {}
    for c in cams:
        yard, _ = frames(pkg.render_gmm, c, 10, "per-step")
        r, per_step[c] = frames(pkg.render_gmm, c, 11, "per-step")
        median_step[c] = r
        print(json.dumps(dict(base, kind="per_step_frame", camera=c, steps=args.steps,
                              warmup=args.warmup, quantile_m11=r, yardstick_range_m10=yard,
                              hit_pixels=int(np.sum(per_step[c] != 0)), **ratios(r, yard))),
              flush=True)

    rec_bytes = n * n * n * K * 3 * ELEM[dt]

    def bake_line(ms):
        first, again = ms[0], ms[1:]
        d = {"first_ms": round(first, 3)}
        if again:
            r = stats(again)
            d.update(rebake=r, GBps=round(rec_bytes / (r["min_ms"] * 1e-3) / 1e9, 1))
            if ceiling:
                d["frac_of_read_ceiling"] = round(d["GBps"] / ceiling, 4)
        return d

    def bake(what, fn):
        with limit(args.step_limit, f"bake {what}"):
            d = bake_line(timed_bakes(torch, s, fn, 1 + args.bakes))
        note(f"bake {what}: {d}")
        return d

    b_stats = bake("stats", pkg.bake_gmm_stats)
    b_range = bake("range", pkg.bake_gmm_range)
    b_quant = bake("quantile", pkg.bake_gmm_quantile)
    assert pkg.gmm_quantile_info()[3] == n and pkg.gmm_range_info()[3] == n
    line = dict(base, kind="bake", record_bytes=rec_bytes, quantile=b_quant, yardstick_range=b_range,
                yardstick_stats=b_stats)
    if "rebake" in b_quant:
        line["time_ratio_to_range"] = round(b_quant["rebake"]["min_ms"] / b_range["rebake"]["min_ms"], 4)
        line["time_ratio_to_stats"] = round(b_quant["rebake"]["min_ms"] / b_stats["rebake"]["min_ms"], 4)
    print(json.dumps(line), flush=True)
    pkg.release_gmm_stats()

    # the spread against the median at the first camera: per step, and the bake
    c0 = cams[0]
    pkg.set_quantile_spread(*SPREAD)   # (drops the median's plane)
    r, spread_step = frames(pkg.render_gmm, c0, 11, "per-step spread")
    print(json.dumps(dict(base, kind="per_step_spread", camera=c0, steps=args.steps,
                          warmup=args.warmup, spread_m11=r, yardstick_median_m11=median_step[c0],
                          **ratios(r, median_step[c0]))), flush=True)
    b_spread = bake("spread", pkg.bake_gmm_quantile)
    line = dict(base, kind="bake_spread", record_bytes=rec_bytes, spread_bake=b_spread,
                yardstick_median_bake=b_quant)
    if "rebake" in b_spread:
        line["time_ratio"] = round(b_spread["rebake"]["min_ms"] / b_quant["rebake"]["min_ms"], 4)
    print(json.dumps(line), flush=True)
    spread_baked, f = frames(pkg.render_gmm_baked, c0, 11, "baked spread")
    spread_mismatch = int(np.sum(f != spread_step))

    # the median's plane again (any set of the quantile dropped the spread's), then
    # frames from the planes with no records resident
    pkg.set_quantile(MEDIAN)
    with limit(args.step_limit, "bake quantile again"):
        pkg.bake_gmm_quantile()
        torch.cuda.synchronize()
    pkg.free_gmm()
    median_baked = {}
    for c in cams:
        yard, _ = frames(pkg.render_gmm_baked, c, 10, "baked")
        r, f = frames(pkg.render_gmm_baked, c, 11, "baked")
        median_baked[c] = r
        print(json.dumps(dict(base, kind="baked_frame", camera=c, steps=args.steps,
                              warmup=args.warmup, quantile_m11=r, yardstick_range_m10=yard,
                              rgba8_mismatch_vs_per_step=int(np.sum(f != per_step[c])),
                              **ratios(r, yard))), flush=True)
    print(json.dumps(dict(base, kind="baked_spread", camera=c0, steps=args.steps,
                          warmup=args.warmup, spread_m11=spread_baked,
                          yardstick_median_m11=median_baked[c0],
                          rgba8_mismatch_vs_per_step=spread_mismatch,
                          **ratios(spread_baked, median_baked[c0]))), flush=True)
    pkg.release_gmm_range()
    pkg.release_gmm_quantile()
    pkg.clear_gmm_range()
    pkg.set_quantile(None)
    pkg.set_stream(None)


if __name__ == "__main__":
    main()
