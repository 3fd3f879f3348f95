#!/usr/bin/env python3
"""The level-crossing query (method 13) against the weighted-bin query (10) on one
scene, in one process (tooling).

Synthesizes the config's float32 volume and, for each view, times N frames of
method 10 and N frames of method 13, both with all weights zero, with HIP events
(one event pair per frame after the warm-up, as bench.py does).  With zero weights
every F is 0, the combine gives (1 - 0) - 1 = 0 and method 10 samples 0 as well:
every sample is transparent, every ray runs its full length, and the two frames are
identical -- k_march_lin and k_march_cross on the same rays.  Times one real query
per view for information (the isovalue 0.3: its rays end early).  Times
vr_bake_weighted and vr_bake_crossing (host clock around the synchronous calls;
both launch k_bake_lin) beside vr_stream_read of the same records, and the baked
method-10 and method-13 frames on planes of the same layout baked with the same
(zero) weights; converts the volume to f16 on the device and does all of it again.
Every frame is also rendered once with d_steps, untimed, for its samples, so times
are reported per frame and per sample.

One JSON line per measurement, appended to --out (default
profiles/crossing/bench_<config>.jsonl); the tables of the run are written to
INDEX.md beside it.

  python tools/bench_crossing.py --config 1024x8 [--views C0 C1 S] [--steps 20]
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

INDEX_HEAD = """# profiles/crossing — the level-crossing query (DESIGN.md §21)

## Code objects — `codeobj_parent.txt`, `codeobj_this.txt`, `codeobj_common.diff`

`python tools/codeobj_list.py libvr.so` of the parent commit's library and of
this one, both built on the CPU for gfx950: kernel name → symbol size,
`vgpr_count`, `sgpr_count`, `private_segment_fixed_size`,
`group_segment_fixed_size`, `kernarg_segment_size`.  632 kernels in the parent,
646 here.  `codeobj_common.diff` holds the parent's rows that are missing or
different here (`grep -vxFf codeobj_this.txt codeobj_parent.txt`): it is empty,
so every `k_march_lin`, `k_march_quant` and `k_march_dist` row is what it was
before the loops of `vr_query.h` took a blend functor.  The 14 rows only here are
the 12 `k_march_cross` instances and the 2 `k_march_cross_plane` ones.

## Workgroups per CU — `occupancy_caps.jsonl`

`python tools/crossing_caps.py`: methods 10 and 13 with zero weights, alternating,
under `VR_WG_PER_CU` caps from none to 3, both dtypes and the three views.  The
ratio at f16 S stays at 1.023-1.028 under every cap, so the workgroups per CU that
the smaller register count of `k_march_cross` allows do not explain it (§21.4).

## Timings — `{jsonl}`

`python tools/bench_crossing.py --config {config}` on one MI355X, one process.
One JSON line per measurement (`what`, `dtype`, `view`, `method`), {warmup}
warm-up + {steps} timed frames each.  The tables below are this run's; DESIGN.md
§21.4 discusses them.  `bench_1024x8_run2.jsonl`, where present, is the same
command in another process; `bench_ab.txt` is `bench.py` of this tree and of the
parent's, alternating.
"""


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
    for what, title in (("per_step_ratio", "Per-step frames, all weights zero: method 13 against "
                                           "method 10 on the same rays"),
                        ("baked_ratio", "Baked frames, planes baked with the same zero weights")):
        sel = [r for r in rows if r["what"] == what]
        if not sel:
            continue
        txt.append(f"\n### {title}\n\n| dtype | view | m13 kernel | m10 kernel | m13 ms | m10 ms | "
                   "frame m13 / m10 | min m13 / m10 | m13 ns / sample | m10 ns / sample | "
                   "same frame |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in sel:
            txt.append(f"| {r['dtype']} | {r['view']} | `{r['m13_kernel']}` | `{r['m10_kernel']}` | "
                       f"{r['m13_ms']} | {r['m10_ms']} | {r['frame_m13_over_m10']} | "
                       f"{r['frame_min_m13_over_m10']} | {r['m13_ns_per_sample']} | "
                       f"{r['m10_ns_per_sample']} | {r['same_frame']} |\n")
    real = [r for r in rows if r["what"] in ("per_step_real", "baked_real")]
    if real:
        txt.append(f"\n### One real query (isovalue {THETA}; for information)\n\n"
                   "| dtype | view | frames from | kernel | ms | samples | ns / sample |\n"
                   "|---|---|---|---|---|---|---|\n")
        for r in real:
            src = "records" if r["what"] == "per_step_real" else "plane"
            txt.append(f"| {r['dtype']} | {r['view']} | {src} | `{r['kernel']}` | {r['mean_ms']} | "
                       f"{r['samples']} | {r['ns_per_sample']} |\n")
    bake = [r for r in rows if r["what"] == "bake"]
    if bake:
        txt.append("\n### Bakes (min of the repetitions, ms; both are k_bake_lin)\n\n"
                   "| dtype | stream read | weighted | crossing | crossing / weighted |\n"
                   "|---|---|---|---|---|\n")
        for r in bake:
            w, x = min(r["bake_weighted_ms"]), min(r["bake_crossing_ms"])
            txt.append(f"| {r['dtype']} | {r['stream_read_min_ms']} | {w} | {x} | "
                       f"{round(x / w, 4)} |\n")
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
    args.out_path = args.out or os.path.join(ROOT, "profiles", "crossing",
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
    base = {"tool": "bench_crossing", "config": args.config, "image": [W, H],
            "steps": args.steps, "warmup": args.warmup}
    rows = []

    def emit(rec):
        rec = dict(base, **rec)
        rows.append(rec)
        with open(args.out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    def measure(what, dtype, view, method):
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
        emit(dict(r, what=what, dtype=dtype, view=view, method=method))
        return r, frame

    def pair(what, dtype, view):
        """method 10 then method 13 on the same rays; the ratio line"""
        a, fa = measure(what, dtype, view, pkg.QUERY_WEIGHTED)
        b, fb = measure(what, dtype, view, pkg.QUERY_CROSSING)
        emit({"what": what + "_ratio", "dtype": dtype, "view": view,
              "m13_kernel": b["kernel"], "m10_kernel": a["kernel"],
              "m13_ms": b["mean_ms"], "m10_ms": a["mean_ms"],
              "frame_m13_over_m10": round(b["mean_ms"] / a["mean_ms"], 4),
              "frame_min_m13_over_m10": round(b["min_ms"] / a["min_ms"], 4),
              "m13_ns_per_sample": b["ns_per_sample"], "m10_ns_per_sample": a["ns_per_sample"],
              "samples_m13": b["samples"], "samples_m10": a["samples"],
              "same_frame": bool(np.array_equal(fa, fb))})

    def timed_call(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def zero_weights():
        pkg.set_crossing_weights(np.zeros(nb, np.float32))
        pkg.set_bin_weights(np.zeros(nb, np.float32))

    pkg.synthesize((n, n, n), nb, bench.SEED)
    for dtype in ("f32", "f16"):
        if dtype == "f16":
            pkg.convert_f16()
        if dtype not in args.dtypes:
            continue
        assert pkg.volume_dtype() == dtype
        pkg.set_layout_budget(None)
        # per-step frames: the parent's k_march_lin against k_march_cross, both on
        # the x rows of the records
        for view in args.views:
            zero_weights()
            pair("per_step", dtype, view)
            pkg.set_isovalue(THETA, nb)
            measure("per_step_real", dtype, view, pkg.QUERY_CROSSING)
        pkg.release_stats()
        # the bakes (the same kernel with either weights), against one streaming
        # read of the same records
        rec_bytes, read_min, read_mean = pkg.stream_read(5)
        zero_weights()
        ms = {"weighted": [], "crossing": []}
        for _ in range(max(args.bake_reps, 1)):
            pkg.release_crossing()
            ms["crossing"].append(timed_call(pkg.bake_crossing))
            pkg.release_weighted()
            ms["weighted"].append(timed_call(pkg.bake_weighted))
        rec = {"what": "bake", "dtype": dtype, "record_bytes": rec_bytes,
               "stream_read_min_ms": round(read_min, 4),
               "stream_read_gbs": round(rec_bytes / (read_min * 1e-3) / 1e9, 1)}
        for k, v in ms.items():
            rec[f"bake_{k}_ms"] = [round(x, 3) for x in v]
            rec[f"bake_{k}_gbs"] = round(rec_bytes / (min(v) * 1e-3) / 1e9, 1)
        emit(rec)
        # baked frames: method 10's plane march against k_march_cross_plane, on two
        # planes of the same layout and contents
        for view in args.views:
            pair("baked", dtype, view)
        pkg.set_isovalue(THETA, nb)  # (drops the crossing plane)
        pkg.bake_crossing()
        for view in args.views:
            measure("baked_real", dtype, view, pkg.QUERY_CROSSING)
        pkg.release_stats()
    pkg.set_crossing_weights(None)
    pkg.set_bin_weights(None)
    pkg.freeCudaBuffers()
    write_index(os.path.join(out_dir, "INDEX.md"), rows, args)


if __name__ == "__main__":
    main()
