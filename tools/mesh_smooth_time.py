#!/usr/bin/env python3
"""Time the mesh adjacency build and the Taubin smoothing (csrc/gpnerf_meshtopo.hip):
  body     -- the stretched icosphere of tools/mesh_raster_time.py / mesh_simplify_time.py (level 7: 327 680 faces, 163 842 vertices,
              valence 6);
  fan      -- N triangles around one vertex (--fan N, 0 to skip): the hub's list holds 2 N half-edges and N + 1 neighbours -- what the
              two quadratic walks cost on a list of that length, and what a lane that sums N + 1 neighbours costs a smoothing pass;
  step     -- each step runs in a child process of its own under its own time limit (--limit seconds): a step that hangs or faults
              ends there and the next one is not started;
  times    -- the adjacency build (frame.mesh_adjacency: the workspace from the caching allocator and the call's launches; no host
              read), one smoothing pass (half of the 1-iteration call's two launches), the 1-iteration and the 10-iteration call, by
              device events, median / min / max of --reps after a warm-up round; the build's kernels by torch's profiler (device-side
              kernel durations) over the same calls, summed per kernel name and divided by the number of calls; the workspace.
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

KERNELS = ("topology_clear_kernel", "face_count_kernel", "scan_sums_kernel", "scan_top_kernel", "scan_apply_kernel", "halfedge_fill_kernel",
           "edge_kernel", "neighbour_fill_kernel", "neighbour_rank_kernel", "vertex_count_kernel", "topology_finish_kernel", "smooth_pass_kernel")


def body_mesh(level):
    import mesh_metric_cases as mm
    v, f = mm.icosphere(level)
    return mm.f32(v.astype(np.float64) * [0.25, 0.2, 0.9]), np.ascontiguousarray(f, dtype=np.int32)


def timed(call, reps):
    import torch
    ms = []
    for rep in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        call()
        e[1].record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e[0].elapsed_time(e[1]))
    return [float(np.median(ms)), float(min(ms)), float(max(ms))]


def step(args):
    import torch
    F = importlib.import_module("gp-nerf_amd.frame")
    L = importlib.import_module("gp-nerf_amd._lib")
    dev = torch.device("cuda:0")
    if args.step == "fan":
        import simplify_cases as sc
        v, f = sc.fan(args.fan)
    else:
        v, f = body_mesh(args.level)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    nv, nf = len(v), len(f)
    pin = args.step != "fan"                                 # (every vertex of the fan is on its border: pinned, nothing would be summed)
    build = lambda: F.mesh_adjacency(tf, nv)
    adj = build()
    torch.cuda.synchronize()
    t_build = timed(build, args.reps)
    per_kernel = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.reps):
                build()
            F.smooth_mesh(tv, adjacency=adj, iterations=1, pin_boundary=pin)
            torch.cuda.synchronize()
        per_kernel = {}
        for ev in prof.events():
            for k in KERNELS:
                if k in ev.name:
                    n = 1 if k == "smooth_pass_kernel" else args.reps
                    per_kernel[k] = per_kernel.get(k, 0.0) + float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0)) / 1e3 / n
                    break
        per_kernel = per_kernel or None
    except Exception as err:                                 # (the whole-call times stand; say why the split is missing)
        per_kernel = {"error": repr(err)}
    t_one = timed(lambda: F.smooth_mesh(tv, adjacency=adj, iterations=1, pin_boundary=pin), args.reps)
    t_ten = timed(lambda: F.smooth_mesh(tv, adjacency=adj, iterations=10, pin_boundary=pin), args.reps)
    out = {"step": args.step, "faces": nf, "vertices": nv, "stats": dict(zip(L.TOPOLOGY_STATS, adj.stats.cpu().tolist())), "pin_boundary": pin,
           "adjacency_ms_median_min_max": t_build, "per_kernel_ms_per_call": per_kernel,
           "smooth_1_iteration_ms_median_min_max": t_one, "smooth_pass_ms": t_one[0] / 2.0,
           "smooth_10_iterations_ms_median_min_max": t_ten,
           "workspace_bytes": int(L.lib().gpnerf_mesh_adjacency_workspace_bytes(nv, nf)),
           "note": "device events around the wrappers' calls (mesh_adjacency: allocation from the caching allocator and 14 launches, no host "
                   "read; smooth_mesh: the output's allocation and 2 launches per iteration); per kernel: profiler, device durations, the "
                   "scans' three kernels summed over the build's two scans, smooth_pass_kernel summed over one iteration's two passes"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fan", type=int, default=100000, help="faces of the hub step (0: skip)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=int, default=7, help="icosphere level: 20 * 4^level faces")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per step")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        return step(args)
    for name in ["body"] + (["fan"] if args.fan > 0 else []):
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
