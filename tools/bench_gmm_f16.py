#!/usr/bin/env python3
"""fp32 against f16 GMM records, one process, one JSON line per scene (tooling).

In-core (default): synthesizes the gmm1024 volume (1024^3 x 16, 1080p) as
float32, times N frames of every requested (camera, method) with HIP events
(one event pair per frame after the warm-up), frees it, synthesizes the same
volume directly as f16 (synthesize_gmm(dtype="f16"): the two never coexist --
together they would not fit one device) and times the same frames again.  Each
line reports both times, both kernels, both algorithmic byte counts (U x 8K /
12K for fp32, U x 4K / 6K for f16, U from gmm_count_footprint), the fraction of
the 8 TB/s HBM peak and how many RGBA8 pixels the f16 frame moves.

--streamed: section 11.4's scene, 512^3 x 16 at 3840x2160 through
stream.GmmStream (host-pinned slabs, 2-buffer HBM ring); reports the frame
times and the host -> device rate each dtype achieved.

  python tools/bench_gmm_f16.py --cameras C0,C1 --methods 1,2 [--steps 20]
  python tools/bench_gmm_f16.py --streamed [--slab 64]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak
REC_BYTES = {"f32": {1: 8, 2: 12}, "f16": {1: 4, 2: 6}}  # per component, by method


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def stats(ms):
    ms = np.asarray(ms)
    return {"mean_ms": round(float(ms.mean()), 4), "median_ms": round(float(np.median(ms)), 4),
            "min_ms": round(float(ms.min()), 4)}


def timed_incore(pkg, torch, s, desc, out, warmup, steps):
    ev = []
    with torch.cuda.stream(s):
        out.zero_()
        for f in range(warmup + steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            pkg.render_gmm(desc)
            e1.record(s)
            if f >= warmup:
                ev.append((e0, e1))
    torch.cuda.synchronize()
    r = stats([a.elapsed_time(b) for a, b in ev])
    r["kernel"] = pkg.last_kernel()
    return r, out.cpu().numpy().view(np.uint32).copy()


def incore(args, pkg, torch, bench):
    n, K, W, H = bench.GMM_CONFIGS[args.config]
    s = torch.cuda.Stream()
    pkg.set_stream(s)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    scenes = [(c, m) for c in args.cameras for m in args.methods]
    res = {sc: {} for sc in scenes}
    frames = {sc: {} for sc in scenes}
    for dt in ("f32", "f16"):
        t0 = time.time()
        pkg.synthesize_gmm((n, n, n), K, bench.SEED, dtype=dt)
        torch.cuda.synchronize()
        assert pkg.gmm_dtype() == dt
        note(f"{dt}: synthesized {n}^3 x {K} in {time.time() - t0:.1f} s")
        for cam, method in scenes:
            desc = pkg.make_desc(out, W, H, bench.camera_matrix(pkg, cam), query_method=method,
                                 volume_size=(1, 1, 1))
            for kv in args.tuning:
                pkg.set_tuning(*kv.split("=", 1))
            r, frames[cam, method][dt] = timed_incore(pkg, torch, s, desc, out, args.warmup,
                                                      args.steps)
            r["U"] = int(pkg.gmm_count_footprint(desc))
            r["footprint_bytes"] = r["U"] * REC_BYTES[dt][method] * K
            r["frac_hbm_peak"] = round(r["footprint_bytes"] / (r["mean_ms"] * 1e-3) / 1e9
                                       / HBM_PEAK_GBS, 4)
            res[cam, method][dt] = r
            note(f"{dt} {cam} m{method}: {r['mean_ms']} ms  {r['kernel']}")
        pkg.free_gmm()  # the fp32 volume goes before the f16 one is made
    for cam, method in scenes:
        r, f = res[cam, method], frames[cam, method]
        line = {"tool": "bench_gmm_f16", "scene": args.config, "volume": [n, n, n], "K": K,
                "camera": cam, "method": method, "image": [W, H], "steps": args.steps,
                "warmup": args.warmup, "tuning": args.tuning,
                "lib": os.path.relpath(pkg.LIB_PATH, ROOT), "f32": r["f32"], "f16": r["f16"],
                "f16_over_f32": round(r["f16"]["mean_ms"] / r["f32"]["mean_ms"], 4),
                "rgba8_mismatch": int(np.sum(f["f32"] != f["f16"])),
                "hit_pixels": int(np.sum(f["f32"] != 0))}
        print(json.dumps(line), flush=True)


def host_volume(pkg, torch, n, K, dt, seed):
    """the synthetic volume in pinned host memory, generated on the device in
    chunks of slices and copied down"""
    tdt, eb = (torch.float16, 2) if dt == "f16" else (torch.float32, 4)
    hip = ctypes.CDLL("libamdhip64.so")
    wm = torch.empty((n, n, n, K, 2), dtype=tdt, pin_memory=True)
    sg = torch.empty((n, n, n, K), dtype=tdt, pin_memory=True)
    chunk = max(1, min(n, int(8e9 // (n * n * K * 3 * eb))))
    for zb in range(0, n, chunk):
        ns = min(chunk, n - zb)
        pkg.synthesize_gmm((n, n, n), K, seed, z_base=zb, nslices=ns, dtype=dt)
        _, _, _, _, pw, ps = pkg.gmm_info()
        torch.cuda.synchronize()
        assert hip.hipMemcpy(ctypes.c_void_p(wm[zb].data_ptr()), ctypes.c_void_p(pw),
                             ctypes.c_size_t(ns * n * n * K * 2 * eb), 2) == 0
        assert hip.hipMemcpy(ctypes.c_void_p(sg[zb].data_ptr()), ctypes.c_void_p(ps),
                             ctypes.c_size_t(ns * n * n * K * eb), 2) == 0
    pkg.free_gmm()
    return wm, sg


def streamed(args, pkg, torch, bench):
    n, K, W, H = 512, 16, 3840, 2160
    cam, method = args.cameras[0], args.methods[0]
    frame = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    desc = pkg.make_desc(frame, W, H, bench.camera_matrix(pkg, cam), query_method=method,
                         volume_size=(1, 1, 1))
    s = torch.cuda.Stream()
    res, frames = {}, {}
    for dt in ("f32", "f16"):
        t0 = time.time()
        wm, sg = host_volume(pkg, torch, n, K, dt, bench.SEED)
        note(f"{dt}: host volume in {time.time() - t0:.1f} s")
        st = pkg.stream.GmmStream(wm, sg, args.slab)
        ev, info = [], None
        for f in range(args.warmup + args.steps):
            frame.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()  # the current stream: GmmStream.render orders its streams after it
            info = st.render(desc, s)
            e1.record(s)
            if f >= args.warmup:
                ev.append((e0, e1))
        torch.cuda.synchronize()
        r = stats([a.elapsed_time(b) for a, b in ev])
        r.update(kernel=pkg.last_kernel(), slabs=info["slabs"],
                 bytes_streamed=int(info["bytes_streamed"]), slab_bytes=int(st.slab_bytes),
                 h2d_GBps=round(info["bytes_streamed"] / (r["mean_ms"] * 1e-3) / 1e9, 2),
                 rays_handed_on=int(info["rays_handed_on"]))
        res[dt] = r
        frames[dt] = frame.cpu().numpy().view(np.uint32).copy()
        note(f"{dt} streamed: {r['mean_ms']} ms, {r['h2d_GBps']} GB/s")
        pkg.set_stream(None)
        del st, wm, sg  # the fp32 host volume and ring go before the f16 ones
        torch.cuda.empty_cache()
    line = {"tool": "bench_gmm_f16", "scene": "streamed", "volume": [n, n, n], "K": K,
            "camera": cam, "method": method, "image": [W, H], "slab_slices": args.slab,
            "steps": args.steps, "warmup": args.warmup,
            "lib": os.path.relpath(pkg.LIB_PATH, ROOT), "f32": res["f32"], "f16": res["f16"],
            "f16_over_f32": round(res["f16"]["mean_ms"] / res["f32"]["mean_ms"], 4),
            "rgba8_mismatch": int(np.sum(frames["f32"] != frames["f16"])),
            "hit_pixels": int(np.sum(frames["f32"] != 0))}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gmm1024", choices=["gmm1024", "gmm96"],
                    help="in-core scene (gmm96: a quick check of the tool)")
    ap.add_argument("--cameras", default="C0", help="comma list of C0, C1")
    ap.add_argument("--methods", default="1", help="comma list of 1, 2")
    ap.add_argument("--steps", type=int, default=20, help="timed frames per dtype (>= 20)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streamed", action="store_true",
                    help="512^3 x 16 at 3840x2160 through stream.GmmStream (first camera / method)")
    ap.add_argument("--slab", type=int, default=64, help="--streamed: slices per slab")
    ap.add_argument("--tuning", nargs="*", default=[], metavar="KEY=VALUE",
                    help="vr_set_tuning knobs for every frame, e.g. VR_WG_PER_CU=3")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be >= 20")
    args.cameras = args.cameras.split(",")
    args.methods = [int(m) for m in args.methods.split(",")]
    if not set(args.cameras) <= {"C0", "C1"} or not set(args.methods) <= {1, 2}:
        ap.error("cameras are C0 / C1, methods 1 / 2")
    args.warmup = max(args.warmup, 1)
    import torch
    import __graft_entry__ as g
    import bench
    pkg = g.load_package()
    torch.cuda.set_device(0)
    (streamed if args.streamed else incore)(args, pkg, torch, bench)


if __name__ == "__main__":
    main()
