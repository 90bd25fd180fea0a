#!/usr/bin/env python3
"""Time the mesh's connected components (csrc/gpnerf_meshcomp.hip):
  body     -- the stretched icosphere of tools/mesh_smooth_time.py (level 7: 327 680 faces, 163 842 vertices): ONE component, so every
              lane of the table kernels targets one row -- the contention case;
  noise    -- the marching-cubes surface of tests/mesh_cases.all_cases_field(): 108 240 faces, 263 components, non-manifold;
  fan      -- N triangles around one vertex (--fan N, 0 to skip): every face's union passes through the hub;
  step     -- each step runs in a child process of its own under its own time limit (--limit seconds): a step that hangs or faults
              ends there and the next one is not started;
  times    -- the adjacency build beside it (frame.mesh_adjacency), the components on a ready adjacency (frame.mesh_components: the
              workspace from the caching allocator and the call's launches; no host read), the emit of the largest component on a
              ready count (frame.filter_components(components=...): its one host read of the two sizes included), by device events,
              median / min / max of --reps after a warm-up round; the components' kernels by torch's profiler (device-side kernel
              durations) over the same calls, summed per kernel name and divided by the number of calls; the workspace.
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

KERNELS = ("init_kernel", "union_kernel", "flatten_kernel", "scan_sums_kernel", "scan_top_kernel", "scan_apply_kernel", "vertex_table_kernel",
           "face_table_kernel", "row_kernel", "mark_kernel", "finish_kernel")
STEPS = ("body", "noise", "fan")


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
    elif args.step == "noise":
        import mesh_cases
        v, f = mesh_cases.marching_cubes_np(mesh_cases.all_cases_field(), 0.02)
        v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
    else:
        v, f = body_mesh(args.level)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    nv, nf = len(v), len(f)
    adj = F.mesh_adjacency(tf, nv)
    count = lambda: F.mesh_components(tf, nv, adjacency=adj, keep="largest")
    comp = count()
    torch.cuda.synchronize()
    t_build = timed(lambda: F.mesh_adjacency(tf, nv), args.reps)
    t_count = timed(count, args.reps)
    t_emit = timed(lambda: F.filter_components(tv, tf, components=comp, want_map=True), args.reps)
    per_kernel = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.reps):
                count()
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
    out = {"step": args.step, "faces": nf, "vertices": nv, "stats": dict(zip(L.COMPONENT_STATS, comp.stats.cpu().tolist())),
           "adjacency_ms_median_min_max": t_build, "components_ms_median_min_max": t_count, "emit_largest_ms_median_min_max": t_emit,
           "per_kernel_ms_per_call": per_kernel, "workspace_bytes": int(L.lib().gpnerf_mesh_components_workspace_bytes(nv, nf)),
           "note": "device events around the wrappers' calls (mesh_components on a ready adjacency: allocation from the caching allocator and "
                   "17 launches, no host read; filter_components on a ready count: the host read of the two sizes, the outputs' allocation and "
                   "3 launches); per kernel: profiler, device durations, the scans' three kernels summed over the call's three scans"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fan", type=int, default=100000, help="faces of the hub step (0: skip)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=int, default=7, help="icosphere level: 20 * 4^level faces")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per step")
    ap.add_argument("--step", default=None, choices=STEPS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        return step(args)
    for name in [s for s in STEPS if s != "fan" or args.fan > 0]:
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
