#!/usr/bin/env python3
"""Time the mesh simplification (csrc/gpnerf_simplify.hip) on a mesh of body-like face count:
  mesh     -- the stretched icosphere of tools/mesh_raster_time.py (level 7: 327 680 faces of about 4.8 mm edges, 0.25 x 0.2 x 0.9 m
              half-extents);
  cells    -- 8 mm and 16 mm (--cells): about a quarter and a sixteenth of the vertices stay;
  fan      -- one more step (--fan N, 0 to skip): N triangles around one vertex, so that ONE cluster's list holds all N faces -- what
              the quadratic rank step and the 64-partial quadric sum cost on a list of that length;
  step     -- each step runs in a child process of its own under its own time limit (--limit seconds): a step that hangs or faults
              ends there and the next one is not started;
  times    -- the whole call (frame.simplify_mesh: count, the read of the two sizes, emit) by device events, median / min / max of
              --reps after a warm-up round; the per-kernel times by torch's profiler (device-side kernel durations) over the same
              calls, summed per kernel name and divided by the number of calls; gpnerf_mesh_rasterize (3 views, 512 x 512) on the
              mesh before and after, for scale; the workspace.
Prints one JSON line per step.  Reads nothing outside the repository."""
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

KERNELS = ("clear_kernel", "vertex_cell_kernel", "face_mark_kernel", "scan_sums_kernel", "scan_top_kernel", "scan_apply_kernel",
           "face_cluster_kernel", "list_fill_kernel", "list_rank_kernel", "position_kernel", "face_verdict_kernel", "finish_kernel",
           "emit_check_kernel", "emit_vertices_kernel", "emit_faces_kernel", "emit_map_kernel")


def body_mesh(level):
    import mesh_metric_cases as mm
    v, f = mm.icosphere(level)
    return mm.f32(v.astype(np.float64) * [0.25, 0.2, 0.9]), np.ascontiguousarray(f, dtype=np.int32)


def step(args):
    import torch
    import raster_cases as rc
    F = importlib.import_module("gp-nerf_amd.frame")
    L = importlib.import_module("gp-nerf_amd._lib")
    dev = torch.device("cuda:0")
    if args.step == "fan":
        import simplify_cases as sc
        v, f = sc.fan(args.fan)
        cell, lo, cells = 1.0, np.zeros(3, dtype=np.float32), [5, 5, 5]
    else:
        v, f = body_mesh(args.level)
        cell = float(args.step)
        lo, cells = F.simplify_grid(v.min(0), v.max(0), cell)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    call = lambda: F.simplify_mesh(tv, tf, cell, lo=lo, cells=cells, want_map=True)
    ov, of, stats, _ = call()
    torch.cuda.synchronize()
    ms = []
    for rep in range(args.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        call()
        e[1].record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e[0].elapsed_time(e[1]))
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
                    break
        per_kernel = per_kernel or None
    except Exception as err:                                 # (the whole-call times stand; say why the split is missing)
        per_kernel = {"error": repr(err)}
    med = lambda x: [float(np.median(x)), float(min(x)), float(max(x))]
    raster = None
    if args.step != "fan":
        side = 512
        Ks, RTs = rc.orbit_cameras(side, side, 3, radius=0.9, distance=3.0, seed=1)
        raster = {}
        for name, (mv, mf) in (("before", (tv, tf)), ("after", (ov, of))):
            t = []
            for rep in range(args.reps + 1):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                F.rasterize_mesh(mv, mf, Ks, RTs, side, side)
                e[1].record()
                torch.cuda.synchronize()
                if rep:
                    t.append(e[0].elapsed_time(e[1]))
            raster[name] = med(t)
    c_cells = (__import__("ctypes").c_int32 * 3)(*cells)
    out = {"step": args.step, "cell": cell, "cells": cells, "faces": int(len(f)), "vertices": int(len(v)),
           "stats": dict(zip(L.SIMPLIFY_STATS, stats.cpu().tolist())), "vertices_kept_share": float(len(ov) / max(len(v), 1)),
           "simplify_ms_median_min_max": med(ms), "per_kernel_ms_per_call": per_kernel,
           "rasterize_3x512x512_ms_median_min_max": raster,
           "workspace_bytes": int(L.lib().gpnerf_mesh_simplify_workspace_bytes(len(v), len(f), c_cells)),
           "note": "device events around the wrapper's call (count, the host read of the two sizes, emit: upper limits); per kernel: "
                   "profiler, device durations, the scans' three kernels summed over the call's four scans"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=float, nargs="+", default=[0.008, 0.016], help="cell edges in the mesh's units (metres)")
    ap.add_argument("--fan", type=int, default=100000, help="faces of the one-cluster fan step (0: skip)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=int, default=7, help="icosphere level: 20 * 4^level faces")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per step")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        return step(args)
    for name in [repr(c) for c in args.cells] + (["fan"] if args.fan > 0 else []):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--level", str(args.level),
               "--fan", str(args.fan)]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": name, "error": f"no result within {args.limit} s: stopped here"}), flush=True)
            return 124
        if r.returncode != 0:
            print(json.dumps({"step": name, "error": f"exit status {r.returncode}: stopped here"}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
