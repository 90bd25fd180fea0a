#!/usr/bin/env python3
"""Time the mesh repair (csrc/gpnerf_meshrepair.hip):
  soup     -- the icosphere of level 7 (327 680 faces) exploded into a triangle soup (983 040 private vertices) with every second face
              flipped: everything welds, one closed patch, half of the faces flip;
  clean    -- the same mesh as it was, vertices shared and wound outward: the cost of a repair that has nothing to do;
  step     -- each step runs in a child process of its own under its own time limit (--limit seconds): a step that hangs or faults
              ends there and the next one is not started;
  times    -- frame.repair_mesh as a whole (the workspace from the caching allocator, the count's launches, the host read of the two
              sizes, the outputs' allocation, the emit's launches) and the two C calls apart on buffers that are there (count: no host
              read; emit: on a ready count), by device events, median / min / max of --reps after a warm-up round; the kernels by
              torch's profiler (device-side kernel durations) over the same count + emit calls, summed per kernel name and divided by
              the number of calls; beside them torch.unique(vertices, dim=0, return_inverse=True) on the same device and input -- the
              only comparable existing way to weld (it sorts, and gives neither the lowest index as representative nor the faces'
              fates, patches or windings); the workspace.
Prints one JSON line per step and appends it to --out (default profiles/r21/mesh_repair_time.jsonl).  Reads nothing outside the
repository."""
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

KERNELS = ("repair_clear_kernel", "repair_vertex_insert_kernel", "repair_vertex_lookup_kernel", "repair_face_insert_kernel",
           "repair_face_lookup_kernel", "repair_box_kernel", "repair_union_kernel", "repair_flatten_kernel", "repair_shared_insert_kernel",
           "repair_shared_lookup_kernel", "repair_patch_kernel", "repair_flip_kernel", "scan_sums_kernel", "scan_top_kernel", "scan_apply_kernel",
           "repair_finish_kernel", "repair_emit_check_kernel", "repair_emit_vertices_kernel", "repair_emit_faces_kernel")
STEPS = ("soup", "clean")


def sphere(level):
    import mesh_metric_cases as mm
    v, f = mm.icosphere(level)
    return mm.f32(v), np.ascontiguousarray(f, dtype=np.int32)


def soup_of(v, f):
    f = f.copy()
    f[1::2] = f[1::2][:, [0, 2, 1]]
    return np.ascontiguousarray(v[f.reshape(-1)]), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)


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
    lib = L.lib()
    dev = torch.device("cuda:0")
    v, f = sphere(args.level)
    if args.step == "soup":
        v, f = soup_of(v, f)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    nv, nf = len(v), len(f)
    ov, of, stats, maps = F.repair_mesh(tv, tf, want_map=True)
    torch.cuda.synchronize()
    row = F.read_mesh_repair(stats)
    t_whole = timed(lambda: F.repair_mesh(tv, tf, want_map=True), args.reps)
    ws = torch.empty((int(lib.gpnerf_mesh_repair_workspace_bytes(nv, nf)),), device=dev, dtype=torch.uint8)
    st = lambda: F._stream_ptr(dev)
    count = lambda: L.check(lib.gpnerf_mesh_repair(tv.data_ptr(), nv, tf.data_ptr(), nf, 0.0, 15, ws.data_ptr(), ws.numel(), stats.data_ptr(), st()),
                            "gpnerf_mesh_repair")
    emit = lambda: L.check(lib.gpnerf_mesh_repair_emit(tv.data_ptr(), nv, tf.data_ptr(), nf, ws.data_ptr(), ws.numel(), ov.data_ptr(), len(ov), of.data_ptr(),
                                                       len(of), maps.vertex_map.data_ptr(), maps.kept_vertices.data_ptr(), maps.face_map.data_ptr(),
                                                       maps.face_fate.data_ptr(), maps.face_patch.data_ptr(), st()), "gpnerf_mesh_repair_emit")
    t_count = timed(count, args.reps)
    t_emit = timed(emit, args.reps)
    t_unique = timed(lambda: torch.unique(tv, dim=0, return_inverse=True), args.reps)
    per_kernel = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.reps):
                count()
                emit()
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
    out = {"step": args.step, "faces": nf, "vertices": nv, "stats": row, "repair_mesh_ms_median_min_max": t_whole,
           "count_ms_median_min_max": t_count, "emit_ms_median_min_max": t_emit, "torch_unique_ms_median_min_max": t_unique,
           "per_kernel_ms_per_call": per_kernel, "workspace_bytes": int(ws.numel()),
           "note": "device events; repair_mesh: allocation from the caching allocator, the count, the host read of the two sizes, the outputs' "
                   "allocation, the emit with all five maps; count / emit: the C calls on buffers that are there; per kernel: profiler, device "
                   "durations, the scans' three kernels summed over the call's two scans; torch.unique(vertices, dim=0, return_inverse=True) "
                   "welds only (sorted order, no face work)"}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=int, default=7, help="icosphere level: 20 * 4^level faces")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "mesh_repair_time.jsonl"))
    ap.add_argument("--step", default=None, choices=STEPS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        return step(args)
    for name in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--level", str(args.level), "--out", args.out]
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
