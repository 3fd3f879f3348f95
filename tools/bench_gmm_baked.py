#!/usr/bin/env python3
"""Baked GMM planes against the per-step GMM march, one process, JSON lines (tooling).

Synthesizes the gmm1024 volume (1024^3 x 16, 1080p) as f16 (or --dtype f32), and

  1. times N per-step frames (render_gmm) of every requested (camera, method)
     with HIP events, one event pair per frame after the warm-up;
  2. bakes the volume (bake_gmm_stats): the first bake, which also allocates and
     zeroes the planes, and --bakes re-bakes of the resident records, each
     between two events; the rate is record bytes (wm + sigma) per second;
  3. frees the records and times the same frames from the planes
     (render_gmm_baked), comparing each with the per-step frame pixel by pixel.

The read ceiling the bake is set against is vr_stream_read of this process: a
1024^3 x 8 float32 histogram volume (34 GB) synthesized and released before the
GMM volume is made (--no-ceiling skips it).

One line per step kind: {"kind": "ceiling"}, {"kind": "bake"} and one
{"kind": "frame"} per scene.  Every GPU step runs under its own time limit: a
step that overruns ends the process at once (exit status 1, the Python stacks
on stderr) and nothing more is started on the GPU.

  python tools/bench_gmm_baked.py --cameras C0,C1,S --methods 1,2 > profiles/gmm_baked/bench_gmm1024_f16.jsonl
  python tools/bench_gmm_baked.py --config gmm96 --no-ceiling     # a quick check of the tool
"""
import argparse
import contextlib
import faulthandler
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ELEM = {"f32": 4, "f16": 2}


def note(msg):
    print(msg, file=sys.stderr, flush=True)


@contextlib.contextmanager
def limit(seconds, what):
    """the step's time limit: a watchdog thread ends the process when it passes
    (it fires even while the main thread waits inside a HIP call)"""
    note(f"[{what}] limit {seconds} s")
    faulthandler.dump_traceback_later(seconds, exit=True)
    t0 = time.time()
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()
    note(f"[{what}] {time.time() - t0:.1f} s")


def stats(ms):
    ms = np.asarray(ms)
    return {"mean_ms": round(float(ms.mean()), 4), "median_ms": round(float(np.median(ms)), 4),
            "min_ms": round(float(ms.min()), 4)}


def timed_frames(pkg, torch, s, render, desc, out, warmup, steps):
    ev = []
    with torch.cuda.stream(s):
        out.zero_()
        for f in range(warmup + steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            render(desc)
            e1.record(s)
            if f >= warmup:
                ev.append((e0, e1))
    torch.cuda.synchronize()
    r = stats([a.elapsed_time(b) for a, b in ev])
    r["kernel"] = pkg.last_kernel()
    return r, out.cpu().numpy().view(np.uint32).copy()


def timed_bake(pkg, torch, s):
    with torch.cuda.stream(s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        pkg.bake_gmm_stats()
        e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gmm1024", choices=["gmm1024", "gmm96"],
                    help="scene (gmm96: a quick check of the tool)")
    ap.add_argument("--dtype", default="f16", choices=["f16", "f32"])
    ap.add_argument("--cameras", default="C0,C1,S", help="comma list of C0, C1, S (side view)")
    ap.add_argument("--methods", default="1,2", help="comma list of 1, 2")
    ap.add_argument("--steps", type=int, default=20, help="timed frames per scene (>= 20)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bakes", type=int, default=3, help="timed re-bakes after the first bake")
    ap.add_argument("--no-ceiling", action="store_true", help="skip the vr_stream_read ceiling")
    ap.add_argument("--step-limit", type=int, default=240,
                    help="seconds each GPU step may take before the process is ended")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be >= 20")
    cams = args.cameras.split(",")
    methods = [int(m) for m in args.methods.split(",")]
    if not set(cams) <= {"C0", "C1", "S"} or not set(methods) <= {1, 2}:
        ap.error("cameras are C0 / C1 / S, methods 1 / 2")
    args.warmup = max(args.warmup, 1)
    import torch
    import __graft_entry__ as g
    import bench
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n, K, W, H = bench.GMM_CONFIGS[args.config]
    dt = args.dtype
    base = {"tool": "bench_gmm_baked", "scene": args.config, "volume": [n, n, n], "K": K,
            "dtype": dt, "image": [W, H], "lib": os.path.relpath(pkg.LIB_PATH, ROOT)}
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
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    scenes = [(c, m) for c in cams for m in methods]
    descs = {(c, m): pkg.make_desc(out, W, H, bench.camera_matrix(pkg, c), query_method=m,
                                   volume_size=(1, 1, 1)) for c, m in scenes}
    per_step, frames = {}, {}
    for sc in scenes:
        with limit(args.step_limit, f"per-step {sc[0]} m{sc[1]}"):
            per_step[sc], frames[sc] = timed_frames(pkg, torch, s, pkg.render_gmm, descs[sc], out,
                                                    args.warmup, args.steps)
        note(f"per-step {sc[0]} m{sc[1]}: {per_step[sc]['mean_ms']} ms  {per_step[sc]['kernel']}")

    rec_bytes = n * n * n * K * 3 * ELEM[dt]
    with limit(args.step_limit, "bake"):
        first = timed_bake(pkg, torch, s)
        again = [timed_bake(pkg, torch, s) for _ in range(args.bakes)]
    dims, _, plane_floats, nbaked = pkg.gmm_stats_info()
    assert tuple(dims) == (n, n, n) and nbaked == n
    bake = {"record_bytes": rec_bytes, "plane_bytes": 2 * 4 * plane_floats,
            "first_ms": round(first, 3), "first_GBps": round(rec_bytes / (first * 1e-3) / 1e9, 1)}
    if again:
        r = stats(again)
        bake.update(rebake=r, GBps=round(rec_bytes / (r["min_ms"] * 1e-3) / 1e9, 1))
        if ceiling:
            bake["frac_of_read_ceiling"] = round(bake["GBps"] / ceiling, 4)
    print(json.dumps(dict(base, kind="bake", **bake)), flush=True)

    pkg.free_gmm()  # the baked frames need no records
    for sc in scenes:
        with limit(args.step_limit, f"baked {sc[0]} m{sc[1]}"):
            r, f = timed_frames(pkg, torch, s, pkg.render_gmm_baked, descs[sc], out, args.warmup,
                                args.steps)
        note(f"baked {sc[0]} m{sc[1]}: {r['mean_ms']} ms  {r['kernel']}")
        print(json.dumps(dict(base, kind="frame", camera=sc[0], method=sc[1], steps=args.steps,
                              warmup=args.warmup, per_step=per_step[sc], baked=r,
                              baked_over_per_step=round(r["mean_ms"] / per_step[sc]["mean_ms"], 4),
                              rgba8_mismatch=int(np.sum(f != frames[sc])),
                              hit_pixels=int(np.sum(f != 0)))), flush=True)
    pkg.release_gmm_stats()
    pkg.set_stream(None)


if __name__ == "__main__":
    main()
