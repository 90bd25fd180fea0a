#!/usr/bin/env python3
"""Time the mesh voxeliser (csrc/gpnerf_voxelize.hip) on a mesh of body-like face count:
  body           -- an icosphere (level 7: 327 680 faces, about what marching cubes gives a body at the project's lattice), stretched
                    to a body's proportions (0.25 x 0.2 x 0.9 m half-extents), on a 5 mm lattice around it with a margin of 4 points:
                    its faces are smaller than a lattice step, so most own no column and the large tier's launch finds an empty list;
  marching_cubes -- that body voxelised, unpacked and meshed by the device's marching cubes at 0.5, voxelised on its own lattice
                    (index units): every vertex sits ON a lattice line, the case the half-open ownership rule is for;
  rules          -- parity and nonzero, each step both;
  step           -- each mesh runs in a child process of its own under its own time limit (--limit seconds): a step that hangs or
                    faults ends there and the next one is not started;
  times          -- the whole call (gpnerf_mesh_voxelize: clear, faces, large faces, resolve) and gpnerf_voxel_stats behind it by device
                    events, medians of --reps after a warm-up round; the per-kernel times by torch's profiler (device-side kernel
                    durations) over the same calls, summed per kernel name and divided by the number of calls; for scale, by device
                    events as well: marching_cubes on the same lattice and rasterize_mesh (3 views, 512 x 512) of the same mesh.
Prints one JSON line per mesh and rule.  Reads nothing outside the repository."""
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

KERNELS = ("voxelize_clear_kernel", "voxelize_faces_kernel", "voxelize_large_kernel", "voxelize_resolve_parity_kernel",
           "voxelize_resolve_nonzero_kernel", "voxel_counts_zero_kernel", "voxel_counts_kernel")
STEPS = ("body", "marching_cubes")
HALF = np.array([0.25, 0.2, 0.9])
SPACING, MARGIN = 0.005, 4


def body_mesh(level):
    import mesh_metric_cases as mm
    v, f = mm.icosphere(level)
    return mm.f32(v.astype(np.float64) * HALF), f


def timed(fn, reps):
    """median, min, max of `reps` calls after one warm-up, by device events, in ms"""
    import torch
    ms = []
    for rep in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        fn()
        e[1].record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e[0].elapsed_time(e[1]))
    return [float(np.median(ms)), float(min(ms)), float(max(ms))]


def step(args, name):
    import torch
    import raster_cases as rc
    F = importlib.import_module("gp-nerf_amd.frame")
    L = importlib.import_module("gp-nerf_amd._lib")
    dev = torch.device("cuda:0")
    v, f = body_mesh(args.level)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    # the lattice around the body: an origin off the mesh's symmetry planes, so that no vertex sits on a column by construction
    step_ = np.full(3, SPACING)
    lo = -(HALF + (MARGIN + 0.37) * SPACING)
    dims = tuple(int(d) for d in np.ceil(2 * (HALF + MARGIN * SPACING) / SPACING).astype(int) + 1)
    if name == "marching_cubes":
        cube = F.voxelize_mesh(tv, tf, lo, step_, dims, rule="nonzero").dense()
        tv, tf = F.marching_cubes(cube, 0.5)
        lo, step_ = np.zeros(3), np.ones(3)
    scale_cube = F.voxelize_mesh(tv, tf, lo, step_, dims, rule="nonzero").dense()
    torch.cuda.synchronize()
    Ks, RTs = rc.orbit_cameras(512, 512, 3, radius=0.9, distance=3.0, seed=1)
    centre = torch.tensor([0.5 * (d - 1) for d in dims], device=dev, dtype=torch.float32)
    world = tv if name == "body" else ((tv - centre) * SPACING).contiguous()      # (for the rasteriser: metres about the origin again)
    scale = {"marching_cubes_same_lattice_ms_median_min_max": timed(lambda: F.marching_cubes(scale_cube, 0.5), args.reps),
             "rasterize_same_mesh_3x512x512_ms_median_min_max": timed(lambda: F.rasterize_mesh(world, tf, Ks, RTs, 512, 512), args.reps)}
    for rule in ("parity", "nonzero"):
        grid = None

        def call():
            nonlocal grid
            grid = F.voxelize_mesh(tv, tf, lo, step_, dims, rule=rule)
            return F.voxel_stats(grid)

        call()
        torch.cuda.synchronize()
        vox_ms = timed(lambda: F.voxelize_mesh(tv, tf, lo, step_, dims, rule=rule), args.reps)
        cnt_ms = timed(lambda: F.voxel_stats(grid), args.reps)
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
        except Exception as err:                             # (the whole-call times stand; say why the split is missing)
            per_kernel = {"error": repr(err)}
        stats = grid.stats.cpu().numpy()
        cd = (importlib.import_module("ctypes").c_int32 * 3)(*dims)
        out = {"mesh": name, "rule": rule, "faces": int(tf.shape[0]), "vertices": int(tv.shape[0]), "dims": list(dims),
               "points": int(np.prod(dims)), "stats": dict(zip(L.VOXEL_STATS, (int(s) for s in stats))),
               "crossings_per_used_face": float(stats[3] / max(stats[0], 1)), "voxelize_ms_median_min_max": vox_ms,
               "voxel_stats_ms_median_min_max": cnt_ms, "per_kernel_ms_per_call": per_kernel,
               "volume_m3": float(stats[5]) * SPACING ** 3, "ellipsoid_volume_m3": float(4.0 / 3.0 * np.pi * np.prod(HALF)),
               "workspace_bytes": int(L.lib().gpnerf_mesh_voxelize_workspace_bytes(int(tf.shape[0]), cd, L.VOXEL_RULES[rule])),
               "note": "device events around the wrapper's calls (they bracket its host work: upper limits); per kernel: profiler, device durations"}
        out.update(scale)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", nargs="+", default=list(STEPS), choices=STEPS)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=int, default=7, help="icosphere level: 20 * 4^level faces")
    ap.add_argument("--limit", type=float, default=180.0, help="seconds per step")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        return step(args, args.step)
    for name in args.meshes:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--level", str(args.level)]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"mesh": name, "error": f"no result within {args.limit} s: stopped here"}), flush=True)
            return 124
        if r.returncode != 0:
            print(json.dumps({"mesh": name, "error": f"exit status {r.returncode}: stopped here"}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
