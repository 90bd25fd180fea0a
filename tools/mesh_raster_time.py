#!/usr/bin/env python3
"""Time the mesh rasteriser (csrc/gpnerf_raster.hip) on a mesh of body-like face count:
  mesh     -- an icosphere (level 7: 327 680 faces, about what marching cubes gives a body at the project's lattice), stretched to a
              body's proportions (0.25 x 0.2 x 0.9 m half-extents); its faces are about a pixel, so the large tier's launch finds an
              empty list and its time is that of its fixed grid;
  cameras  -- 3 views on an orbit of 3 m, the mesh filling 0.8 of the image's height;
  sizes    -- 512 x 512 and 1024 x 1024 (--sizes);
  step     -- each size runs in a child process of its own under its own time limit (--limit seconds): a step that hangs or faults
              ends there and the next one is not started;
  times    -- the whole call (gpnerf_mesh_rasterize: clear, faces, large faces, resolve) and gpnerf_silhouette_stats behind it by
              device events, medians of --reps after a warm-up round; the per-kernel times by torch's profiler (device-side kernel
              durations) over the same calls, summed per kernel name and divided by the number of calls.
Prints one JSON line per size.  Reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("raster_clear_kernel", "raster_faces_kernel", "raster_large_kernel", "raster_resolve_kernel", "silhouette_zero_kernel",
           "silhouette_count_kernel")


def body_mesh(level):
    import mesh_metric_cases as mm
    v, f = mm.icosphere(level)
    return mm.f32(v.astype(np.float64) * [0.25, 0.2, 0.9]), f


def step(args, side):
    import torch
    import raster_cases as rc
    F = importlib.import_module("gp-nerf_amd.frame")
    dev = torch.device("cuda:0")
    v, f = body_mesh(args.level)
    Ks, RTs = rc.orbit_cameras(side, side, 3, radius=0.9, distance=3.0, seed=1)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    masks = None

    def call():
        res = F.rasterize_mesh(tv, tf, Ks, RTs, side, side)
        return res, (F.silhouette_stats(res["face_id"], masks) if masks is not None else None)

    res, _ = call()
    masks = (res["face_id"] >= 0).to(torch.uint8)
    torch.cuda.synchronize()
    raster_ms, sil_ms = [], []
    for rep in range(args.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        res = F.rasterize_mesh(tv, tf, Ks, RTs, side, side)
        e[1].record()
        counts = F.silhouette_stats(res["face_id"], masks)
        e[2].record()
        torch.cuda.synchronize()
        if rep:
            raster_ms.append(e[0].elapsed_time(e[1]))
            sil_ms.append(e[1].elapsed_time(e[2]))
    per_kernel = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.reps):
                call()
            torch.cuda.synchronize()
        per_kernel = {}
        for ev in prof.events():
            for k in KERNELS:
                if k in ev.name:
                    per_kernel[k] = per_kernel.get(k, 0.0) + float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0)) / 1e3 / args.reps
        per_kernel = per_kernel or None
    except Exception as err:                                 # (the whole-call times stand; say why the split is missing)
        per_kernel = {"error": repr(err)}
    stats = res["stats"].cpu().numpy()
    med = lambda x: [float(np.median(x)), float(min(x)), float(max(x))]
    out = {"size": side, "views": 3, "faces": int(len(f)), "vertices": int(len(v)), "stats_drawn_skipv_skipa_pixels": stats.tolist(),
           "pixels_per_drawn_face": float(stats[:, 3].sum() / max(stats[:, 0].sum(), 1)),
           "rasterize_ms_median_min_max": med(raster_ms), "silhouette_stats_ms_median_min_max": med(sil_ms),
           "per_kernel_ms_per_call": per_kernel, "silhouette_counts": counts.cpu().numpy().tolist(),
           "workspace_bytes": int(importlib.import_module("gp-nerf_amd._lib").lib().gpnerf_mesh_raster_workspace_bytes(len(f), 3, side, side)),
           "note": "device events around the wrapper's calls (they bracket its host work: upper limits); per kernel: profiler, device durations"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=int, default=7, help="icosphere level: 20 * 4^level faces")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per step")
    ap.add_argument("--step", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        return step(args, args.step)
    for side in args.sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(side), "--reps", str(args.reps), "--level", str(args.level)]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"size": side, "error": f"no result within {args.limit} s: stopped here"}), flush=True)
            return 124
        if r.returncode != 0:
            print(json.dumps({"size": side, "error": f"exit status {r.returncode}: stopped here"}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
