#!/usr/bin/env python3
"""Time the truncated signed distance field (csrc/gpnerf_sdf.hip) on the body-sized golden mesh (tests/golden/mesh/mesh_body.npz:
79 948 faces, marching cubes of its padded cube) on that cube's own lattice (index units: lo 0, step 1), at bands of 2, 4 and 8 steps:
  mesh_sdf   -- gpnerf_mesh_sdf with the voxels given (clear, faces, large faces, resolve) by device events; per launch by torch's
                profiler (device-side kernel durations) over the same calls;
  yardstick  -- the same field by existing code: point_mesh_distance over ALL lattice points with max_dist = band and the grid
                given (built outside the timed region); the two are compared bit for bit, and the ratio is recorded;
  beside it  -- voxelize_mesh (the signs), SdfGrid.sample at 200 000 points, SdfGrid.offset_mesh(0) (a negation, marching cubes
                with its one host read, the map to the lattice's frame);
  work       -- from the stats: lattice points visited per used face, (face, point) pairs within the band per lattice point (the
                atomics issued are at most that many).
Each band runs in a child process of its own under its own time limit (--limit seconds): a step that hangs or faults ends there and
the next one is not started.  Prints one JSON line per band: medians of --reps after a warm-up, with min and max.  Reads nothing
outside the repository."""
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

KERNELS = ("sdf_clear_kernel", "sdf_faces_kernel", "sdf_large_kernel", "sdf_resolve_kernel")
BANDS = (2.0, 4.0, 8.0)


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


def step(args, band):
    import torch
    import sdf_cases as sc
    F = importlib.import_module("gp-nerf_amd.frame")
    L = importlib.import_module("gp-nerf_amd._lib")
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "mesh", "mesh_body.npz"))
    cube = torch.from_numpy(np.ascontiguousarray(z["cube"], dtype=np.float32)).to(dev)
    tv, tf = F.marching_cubes(cube, float(z["iso"]))
    dims, lo, unit = tuple(cube.shape), np.zeros(3), np.ones(3)
    voxels = F.voxelize_mesh(tv, tf, lo, unit, dims, rule="nonzero")
    grid = None

    def call():
        nonlocal grid
        grid = F.mesh_sdf(tv, tf, lo, unit, dims, band, voxels=voxels, want_face=True)

    call()
    torch.cuda.synchronize()
    sdf_ms = timed(call, args.reps)
    vox_ms = timed(lambda: F.voxelize_mesh(tv, tf, lo, unit, dims, rule="nonzero"), args.reps)
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
    # the yardstick: one query per lattice point through the mesh's grid
    pts = torch.from_numpy(sc.lattice_points(lo, unit, dims).reshape(-1, 3)).to(dev)
    mesh_grid = F.build_mesh_grid(tv, tf)
    res = None

    def listed():
        nonlocal res
        res = F.point_mesh_distance(pts, grid=mesh_grid, max_dist=band)

    list_ms = timed(listed, args.list_reps)
    d = torch.where(torch.isinf(res["dist"]), torch.full_like(res["dist"], grid.band), res["dist"]).reshape(dims)
    same = bool(torch.equal(grid.values.abs().view(torch.int32), d.view(torch.int32)) and torch.equal(grid.face, res["face"].reshape(dims)))
    rng = np.random.default_rng(0)
    samples = torch.from_numpy((rng.uniform(0, np.array(dims) - 1, (args.samples, 3))).astype(np.float32)).to(dev)
    sample_ms = timed(lambda: grid.sample(samples), args.reps)
    offset_ms = timed(lambda: grid.offset_mesh(0.0), args.reps)
    ov, of = grid.offset_mesh(0.0)
    stats = dict(zip(L.SDF_STATS, (int(s) for s in grid.stats.cpu().numpy())))
    points = int(np.prod(dims))
    print(json.dumps({"band_steps": band, "faces": int(tf.shape[0]), "vertices": int(tv.shape[0]), "dims": list(dims), "points": points,
                      "stats": stats, "points_visited_per_used_face": stats["visited"] / max(stats["used"], 1),
                      "pairs_in_band_per_lattice_point": stats["pairs"] / points,
                      "pairs_in_band_per_point_in_band": stats["pairs"] / max(stats["in_band"], 1),
                      "mesh_sdf_ms_median_min_max": sdf_ms, "per_kernel_ms_per_call": per_kernel,
                      "point_mesh_distance_all_points_ms_median_min_max": list_ms, "list_reps": args.list_reps, "list_form_over_scatter_form": list_ms[0] / sdf_ms[0],
                      "bit_equal_to_the_list_form": same, "voxelize_mesh_ms_median_min_max": vox_ms,
                      "sample_points": args.samples, "sample_ms_median_min_max": sample_ms,
                      "offset_mesh_ms_median_min_max": offset_ms, "offset_mesh_faces": int(of.shape[0]),
                      "workspace_bytes": int(L.lib().gpnerf_mesh_sdf_workspace_bytes(int(tf.shape[0]), (importlib.import_module("ctypes").c_int32 * 3)(*dims))),
                      "note": "device events around the wrapper's calls (they bracket its host work: upper limits); per kernel: profiler, device "
                              "durations; offset_mesh holds marching cubes' one host read"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bands", nargs="+", type=float, default=list(BANDS), help="in lattice steps")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--list-reps", type=int, default=7, help="repetitions of the yardstick (tens of milliseconds per call)")
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--limit", type=float, default=150.0, help="seconds per band")
    ap.add_argument("--step", type=float, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        return step(args, args.step)
    for band in args.bands:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(band), "--reps", str(args.reps), "--samples", str(args.samples), "--list-reps",
               str(args.list_reps)]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"band_steps": band, "error": f"no result within {args.limit} s: stopped here"}), flush=True)
            return 124
        if r.returncode != 0:
            print(json.dumps({"band_steps": band, "error": f"exit status {r.returncode}: stopped here"}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
