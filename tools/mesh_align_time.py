#!/usr/bin/env python3
"""Time the registration (csrc/gpnerf_align.hip) on a marching-cubes-sized mesh, in one process:
  align    -- frame.align_mesh of the body-sized golden mesh (tests/golden/mesh/mesh_body.npz), rotated 3 degrees about its centre
              and shifted by a voxel, onto itself: --samples source samples x --iterations steps, the target's grid built outside
              the timed region (mesh_metrics builds it anyway) and inside it;
  phases   -- per iteration: transform_points, point_mesh_distance(want_closest), align_step: device-event times of one iteration;
  fit      -- frame.rigid_fit at --pairs pairs, with weights and scale;
  graph    -- the whole loop captured into a graph and replayed (no launch overhead).
Prints one JSON line: medians of --reps after one warm-up round, with min and max.  Reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = importlib.import_module("gp-nerf_amd.frame")
L = importlib.import_module("gp-nerf_amd._lib")
import align_cases as ac  # noqa: E402


def golden_mesh(name, dev):
    z = np.load(os.path.join(ROOT, "tests", "golden", "mesh", name + ".npz"))
    return F.marching_cubes(torch.from_numpy(np.ascontiguousarray(z["cube"], dtype=np.float32)).to(dev), float(z["iso"]))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=100000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gv, gf = golden_mesh("mesh_body", dev)
    centre = gv.mean(dim=0).cpu().numpy().astype(np.float64)
    A = np.hstack([ac.rotation((1.0, 2.0, -1.0), 3.0), np.zeros((3, 1))])
    A[:, 3] = centre + [1.0, 0.0, 0.0] - A[:, :3] @ centre
    sv = F.transform_points(gv, F.align_init(gv, init=A))
    grid = F.build_mesh_grid(gv, gf, check=False)
    times = {"align_given_grid": [], "align_with_grid_build": [], "transform": [], "distance": [], "step": [], "rigid_fit": [], "graph_replay": []}
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.normal(size=(args.pairs, 3)).astype(np.float32)).to(dev)
    dst = F.transform_points(src, F.align_init(src, init=A))
    w = torch.from_numpy(rng.uniform(0.5, 2.0, args.pairs).astype(np.float32)).to(dev)
    res = None
    for rep in range(args.reps + 1):
        t_given, res = timed(lambda: F.align_mesh((sv, gf), None, iterations=args.iterations, n_samples=args.samples, grid=grid))
        t_build, _ = timed(lambda: F.align_mesh((sv, gf), (gv, gf), iterations=args.iterations, n_samples=args.samples))
        pts = F.sample_surface(sv, gf, args.samples, want_face=False, want_normal=False)["points"]
        ws, slot, cur = F.align_workspace(dev), F.align_init(pts), torch.empty_like(pts)
        t_tr, _ = timed(lambda: F.transform_points(pts, slot, out=cur))
        t_d, near = timed(lambda: F.point_mesh_distance(cur, grid=grid, want_closest=True))
        t_s, _ = timed(lambda: F.align_step(cur, near, gv, gf, slot, workspace=ws))
        t_fit, fit = timed(lambda: F.rigid_fit(src, dst, w, scale=True, workspace=ws))
        if rep:
            for k, v in (("align_given_grid", t_given), ("align_with_grid_build", t_build), ("transform", t_tr), ("distance", t_d), ("step", t_s),
                         ("rigid_fit", t_fit)):
                times[k].append(v)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = F.align_mesh((sv, gf), None, iterations=args.iterations, n_samples=args.samples, grid=grid)
    for rep in range(args.reps + 1):
        t, _ = timed(g.replay)
        if rep:
            times["graph_replay"].append(t)
    same = captured["transform"].cpu().numpy().tobytes() == res["transform"].cpu().numpy().tobytes()
    t, f = F.read_transform(res["transform"]), F.read_transform(fit)
    truth = np.hstack([A[:, :3].T, (-A[:, :3].T @ A[:, 3])[:, None]])
    print(json.dumps({"faces": int(gf.shape[0]), "samples": args.samples, "iterations": args.iterations, "pairs": args.pairs,
                      "ms": {k: stats(v) for k, v in times.items()}, "graph_replay_same_bits": same,
                      "align": {"status": t["status"], "rms": t["rms"], "rotation_deg": t["rotation_deg"], "used": t["used"],
                                "max_matrix_error": float(np.abs(t["matrix"][:3] - truth).max()),
                                "rms_history": [float(x) for x in res["history"][:, 0].cpu().numpy()]},
                      "fit": {"status": f["status"], "rms": f["rms"], "max_matrix_error": float(np.abs(f["matrix"][:3] - A).max())},
                      "note": "device events around the calls (launch overhead included, but for graph_replay); medians of --reps after one "
                              "warm-up round"}))


if __name__ == "__main__":
    main()
