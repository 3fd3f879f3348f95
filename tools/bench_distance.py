#!/usr/bin/env python3
"""The distribution-distance query (method 12) against the weighted-bin query (10)
on one scene, in one process (tooling).

Synthesizes the config's float32 volume and, for each view and metric, times N
frames of method 12 with the target h = 0 and N frames of method 10 with the
weights that give it the distance frame's own rays, with HIP events (one event
pair per frame after the warm-up, as bench.py does):

    L1  with h = 0  is  0.5 * sum p_i            method 10 with w_i = 0.5
    KS  with h = 0  is  max_i of the prefix sums method 10 with w_i = 1 (the last one)
    EMD with h = 0  is  sum of them / B          method 10 with w_i = (B - i) / B

(identical frames on f16 for L1, the same rays up to rounding otherwise).  Times
one real query for information (the target the mean record of a box at the
centre, L1, similarity on: its rays differ).  Times vr_bake_weighted and
vr_bake_distance (host clock around the synchronous calls) beside vr_stream_read
of the same records, and the baked method-10 and method-12 frames, both on x-row
planes of the same layout; converts the volume to f16 on the device and does all
of it again.  Every frame is also rendered once with d_steps, untimed, for its
samples, so times are reported per frame and per sample.

One JSON line per measurement, appended to --out (default
profiles/distance/bench_<config>.jsonl); the tables of the run are written to
INDEX.md beside it.

  python tools/bench_distance.py --config 1024x8 [--views C0 C1 S] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("l1", "ks", "emd")

INDEX_HEAD = """# profiles/distance — the distribution-distance query (DESIGN.md §20)

## Code objects — `codeobj_parent.txt`, `codeobj_this.txt`, `codeobj_common.diff`

`python tools/codeobj_list.py libvr.so` of the parent commit's library and of
this one, both built on the CPU for gfx950: kernel name → symbol size,
`vgpr_count`, `sgpr_count`, `private_segment_fixed_size`,
`group_segment_fixed_size`, `kernarg_segment_size`.  560 kernels in the parent,
632 here.  `codeobj_common.diff` holds the parent's rows that are missing or
different here (`grep -vxFf codeobj_this.txt codeobj_parent.txt`): it is empty.
The 72 rows only here are the `k_march_dist` and `k_bake_dist` instances.

## Occupancy caps — `caps_codeobj.txt`

The `k_march_dist` rows of three builds with other `amdgpu_waves_per_eu` caps
(`-D'VR_DIST_MAXWAVES(B)=…'`) that differ from the shipped build's.  Not timed.

## Timings — `{jsonl}`

`python tools/bench_distance.py --config {config}` on one MI355X, one process.
One JSON line per measurement (`what`, `dtype`, `view`, `metric`, `method`),
{warmup} warm-up + {steps} timed frames each.  The tables below are this run's;
DESIGN.md §20.4 discusses them.  `bench_1024x8_run2.jsonl`, where present, is the
same command in another process; `bench_ab.txt` is `bench.py` of this tree and of
the parent's, alternating.
"""


def method10_weights(metric, nb):
    """the method-10 weights whose frame has the rays of the distance frame with h = 0"""
    if metric == "l1":
        return np.full(nb, 0.5, np.float32)
    if metric == "ks":
        return np.ones(nb, np.float32)
    return ((nb - np.arange(nb, dtype=np.float32)) / np.float32(nb)).astype(np.float32)


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


def write_index(path, rows, args):
    """INDEX.md: the fixed head and the tables of this run"""
    txt = [INDEX_HEAD.format(jsonl=os.path.basename(args.out_path), config=args.config,
                             warmup=args.warmup, steps=args.steps)]
    step = [r for r in rows if r["what"] == "per_step_ratio"]
    if step:
        txt.append("\n### Per-step frames, h = 0 against method 10 with the same rays\n\n"
                   "| dtype | view | metric | m12 ms | m10 ms | frame m12 / m10 | "
                   "m12 ns / sample | m10 ns / sample | same frame |\n"
                   "|---|---|---|---|---|---|---|---|---|\n")
        for r in step:
            txt.append(f"| {r['dtype']} | {r['view']} | {r['metric']} | {r['m12_ms']} | "
                       f"{r['m10_ms']} | {r['frame_m12_over_m10']} | {r['m12_ns_per_sample']} | "
                       f"{r['m10_ns_per_sample']} | {r['same_frame']} |\n")
    real = [r for r in rows if r["what"] == "per_step_real"]
    if real:
        txt.append("\n### One real query (the mean record of a box, L1, similarity on; for "
                   "information)\n\n| dtype | view | ms | samples | ns / sample |\n"
                   "|---|---|---|---|---|\n")
        for r in real:
            txt.append(f"| {r['dtype']} | {r['view']} | {r['mean_ms']} | {r['samples']} | "
                       f"{r['ns_per_sample']} |\n")
    bake = [r for r in rows if r["what"] == "bake"]
    if bake:
        txt.append("\n### Bakes (min of the repetitions, ms)\n\n| dtype | stream read | weighted | "
                   "L1 | KS | EMD | L1 / weighted | KS / weighted | EMD / weighted |\n"
                   "|---|---|---|---|---|---|---|---|---|\n")
        for r in bake:
            w = min(r["bake_weighted_ms"])
            d = {m: min(r[f"bake_{m}_ms"]) for m in METRICS}
            txt.append(f"| {r['dtype']} | {r['stream_read_min_ms']} | {w} | {d['l1']} | {d['ks']} | "
                       f"{d['emd']} | {round(d['l1'] / w, 4)} | {round(d['ks'] / w, 4)} | "
                       f"{round(d['emd'] / w, 4)} |\n")
    baked = [r for r in rows if r["what"] == "baked_ratio"]
    if baked:
        txt.append("\n### Baked frames (L1 with h = 0 against method 10 with w = 0.5)\n\n"
                   "| dtype | view | m12 ms | m10 ms | frame m12 / m10 | same frame |\n"
                   "|---|---|---|---|---|---|\n")
        for r in baked:
            txt.append(f"| {r['dtype']} | {r['view']} | {r['m12_ms']} | {r['m10_ms']} | "
                       f"{r['frame_m12_over_m10']} | {r['same_frame']} |\n")
    with open(path, "w") as f:
        f.write("".join(txt))


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
    args.out_path = args.out or os.path.join(ROOT, "profiles", "distance",
                                             f"bench_{args.config}.jsonl")
    out_dir = os.path.dirname(os.path.abspath(args.out_path))
    os.makedirs(out_dir, exist_ok=True)
    import torch
    import __graft_entry__ as g
    import bench
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n, nb, W, H = bench.CONFIGS[args.config]
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    steps_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    base = {"tool": "bench_distance", "config": args.config, "image": [W, H],
            "steps": args.steps, "warmup": args.warmup}
    rows = []

    def emit(rec):
        rec = dict(base, **rec)
        rows.append(rec)
        with open(args.out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    def measure(what, dtype, view, method, metric):
        m = bench.camera_matrix(pkg, view)
        desc = pkg.make_desc(out, W, H, m, query_method=method, volume_size=(n, n, n))
        r = frames(pkg, torch, desc, max(args.warmup, 1), args.steps)
        frame = out.cpu().numpy().copy()
        # the same frame once more with d_steps, untimed: its samples
        pkg.render(pkg.make_desc(out, W, H, m, query_method=method, volume_size=(n, n, n),
                                 d_steps=steps_buf))
        torch.cuda.synchronize()
        s = steps_buf.cpu().numpy()
        r["samples"] = int(s[s > 0].sum())
        r["rays"] = int((s >= 0).sum())
        r["ns_per_sample"] = round(r["mean_ms"] * 1e6 / max(r["samples"], 1), 5)
        emit(dict(r, what=what, dtype=dtype, view=view, method=method, metric=metric))
        return r, frame

    def pair(what, dtype, view, metric):
        """method 10 then method 12 on the same rays; the ratio line"""
        a, fa = measure(what, dtype, view, pkg.QUERY_WEIGHTED, metric)
        b, fb = measure(what, dtype, view, pkg.QUERY_DISTANCE, metric)
        emit({"what": what + "_ratio", "dtype": dtype, "view": view, "metric": metric,
              "m12_ms": b["mean_ms"], "m10_ms": a["mean_ms"],
              "frame_m12_over_m10": round(b["mean_ms"] / a["mean_ms"], 4),
              "frame_min_m12_over_m10": round(b["min_ms"] / a["min_ms"], 4),
              "m12_ns_per_sample": b["ns_per_sample"], "m10_ns_per_sample": a["ns_per_sample"],
              "sample_m12_over_m10": round(b["ns_per_sample"] / a["ns_per_sample"], 4),
              "samples_m12": b["samples"], "samples_m10": a["samples"],
              "same_frame": bool(np.array_equal(fa, fb))})

    def timed_call(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def against_zero(metric):
        pkg.set_query_target(np.zeros(nb, np.float32), metric)
        pkg.set_bin_weights(method10_weights(metric, nb))

    pkg.synthesize((n, n, n), nb, bench.SEED)
    c = n // 2
    box = ((c - 4, c - 4, c - 4), (c + 4, c + 4, c + 4))
    for dtype in ("f32", "f16"):
        if dtype == "f16":
            pkg.convert_f16()
        if dtype not in args.dtypes:
            continue
        assert pkg.volume_dtype() == dtype
        pkg.set_layout_budget(None)
        # per-step frames: the parent's k_march_lin against k_march_dist, both on
        # the x rows of the records
        for view in args.views:
            for metric in METRICS:
                against_zero(metric)
                pair("per_step", dtype, view, metric)
            pkg.set_query_target_region(*box, metric="l1", similarity=True)
            measure("per_step_real", dtype, view, pkg.QUERY_DISTANCE, "l1")
        pkg.release_stats()
        # the bakes, against one streaming read of the same records
        rec_bytes, read_min, read_mean = pkg.stream_read(5)
        ms = {"weighted": []}
        for metric in METRICS:
            against_zero(metric)
            ms[metric] = []
            for _ in range(max(args.bake_reps, 1)):
                pkg.release_distance()
                ms[metric].append(timed_call(pkg.bake_distance))
                if metric == "l1":
                    pkg.release_weighted()
                    ms["weighted"].append(timed_call(pkg.bake_weighted))
        rec = {"what": "bake", "dtype": dtype, "record_bytes": rec_bytes,
               "stream_read_min_ms": round(read_min, 4),
               "stream_read_gbs": round(rec_bytes / (read_min * 1e-3) / 1e9, 1)}
        for k, v in ms.items():
            rec[f"bake_{k}_ms"] = [round(x, 3) for x in v]
            rec[f"bake_{k}_gbs"] = round(rec_bytes / (min(v) * 1e-3) / 1e9, 1)
        emit(rec)
        # baked frames: the same plane march on two planes of the same layout
        against_zero("l1")
        pkg.bake_weighted()
        pkg.bake_distance()
        for view in args.views:
            pair("baked", dtype, view, "l1")
        pkg.release_stats()
    pkg.freeCudaBuffers()
    write_index(os.path.join(out_dir, "INDEX.md"), rows, args)


if __name__ == "__main__":
    main()
