#!/usr/bin/env python3
"""Time the mesh metrics (csrc/gpnerf_meshdist.hip) on the two body-sized golden meshes, in one process:
  pairs    -- the marching-cubes meshes of tests/golden/mesh/mesh_body.npz and mesh_trained.npz against each other (both directions),
              and each against itself shifted by half a voxel (0.5 index units along x);
  phases   -- grid build (both meshes), sampling (both), each distance direction (with cosines), the four stats: device-event times;
  brute    -- the brute-force form of the distance at the same size;
  numpy    -- the float64 numpy restatement (tests/mesh_metric_cases.py: every face, no grid) on --numpy-queries of the queries,
              scaled to the full count (wall clock, the device idle meanwhile);
  grid     -- the cells chosen and the entries used over the capacity.
Prints one JSON line per pair: medians of --reps after one warm-up round, with min and max.  Reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = importlib.import_module("gp-nerf_amd.frame")
L = importlib.import_module("gp-nerf_amd._lib")
import mesh_metric_cases as mm  # noqa: E402

PHASES = ("grid_build", "sampling", "dist_pred_to_gt", "dist_gt_to_pred", "stats")


def golden_mesh(name, dev):
    z = np.load(os.path.join(ROOT, "tests", "golden", "mesh", name + ".npz"))
    return F.marching_cubes(torch.from_numpy(np.ascontiguousarray(z["cube"], dtype=np.float32)).to(dev), float(z["iso"]))


def one_round(pred, gt, n, th, brute):
    """the phases of mesh_metrics with an event between them -> (ms per phase, brute-force ms or None, grids, slots)"""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1 + 2)]
    e[0].record()
    g_gt = F.build_mesh_grid(*gt, check=False)
    g_pred = F.build_mesh_grid(*pred, check=False)
    e[1].record()
    sp = F.sample_surface(*pred, n, seed=0, want_face=False)
    sg = F.sample_surface(*gt, n, seed=1, want_face=False)
    e[2].record()
    a = F.point_mesh_distance(sp["points"], grid=g_gt, query_normals=sp["normal"])
    e[3].record()
    b = F.point_mesh_distance(sg["points"], grid=g_pred, query_normals=sg["normal"])
    e[4].record()
    slots = torch.empty((4, L.DIST_DOUBLES), device=sp["points"].device, dtype=torch.float64)
    for k, (values, t) in enumerate(((a["dist"], th), (b["dist"], th), (a["cosine"], ()), (b["cosine"], ()))):
        F.distance_stats(values, t, out=slots[k])
    e[5].record()
    if brute:
        e[6].record()
        c = F.point_mesh_distance(sp["points"], *gt, query_normals=sp["normal"])
        e[7].record()
    torch.cuda.synchronize()
    ms = {p: e[k].elapsed_time(e[k + 1]) for k, p in enumerate(PHASES)}
    same = None
    if brute:
        same = bool(torch.equal(c["dist"].view(torch.int32), a["dist"].view(torch.int32)) and torch.equal(c["face"], a["face"]))
    return ms, (e[6].elapsed_time(e[7]) if brute else None), same, (g_gt, g_pred), slots, sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--numpy-queries", type=int, default=16)
    ap.add_argument("--no-brute", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    th = (0.5, 1.0, 2.0)                                      # index units: half a voxel, one, two
    body, trained = golden_mesh("mesh_body", dev), golden_mesh("mesh_trained", dev)
    shifted = lambda m: (m[0] + torch.tensor([0.5, 0.0, 0.0], device=dev), m[1])
    pairs = (("body_vs_trained", body, trained), ("body_vs_shifted", body, shifted(body)), ("trained_vs_shifted", trained, shifted(trained)))
    for name, pred, gt in pairs:
        times = {p: [] for p in PHASES}
        brute_ms = []
        for rep in range(args.reps + 1):
            ms, b, same, grids, slots, sp = one_round(pred, gt, args.samples, th, not args.no_brute)
            if rep:
                for p in PHASES:
                    times[p].append(ms[p])
                if b is not None:
                    brute_ms.append(b)
        med = {p: float(np.median(v)) for p, v in times.items()}
        res = {"pair": name, "faces": [int(pred[1].shape[0]), int(gt[1].shape[0])], "samples": args.samples,
               "ms": med, "ms_min_max": {p: [float(min(v)), float(max(v))] for p, v in times.items()}, "ms_total": float(sum(med.values())),
               "metrics": {k: v for k, v in F.read_mesh_metrics(slots, th).items()}}
        for side, g in zip(("gt", "pred"), grids):
            h = g.header()
            res["grid_" + side] = {"cells": h["cells"], "n_cells": h["n_cells"], "entries": h["needed"], "entry_cap": h["entry_cap"],
                                   "entries_per_face": h["needed"] / max(h["valid"], 1), "status": h["status"]}
        if brute_ms:
            res["brute_ms"] = float(np.median(brute_ms))
            res["brute_ms_min_max"] = [float(min(brute_ms)), float(max(brute_ms))]
            res["brute_equals_grid"] = same
            res["brute_vs_grid"] = res["brute_ms"] / med["dist_pred_to_gt"]
        if args.numpy_queries:
            q = sp["points"][:: max(1, args.samples // args.numpy_queries)][:args.numpy_queries].cpu().numpy()
            v, f = gt[0].cpu().numpy(), gt[1].cpu().numpy()
            t0 = time.perf_counter()
            mm.all_distances(q, v, f, np.float64).min(axis=1)
            dt = time.perf_counter() - t0
            res["numpy_ms_scaled"] = dt * 1e3 * args.samples / len(q)
            res["numpy_queries"] = len(q)
            res["numpy_vs_grid"] = res["numpy_ms_scaled"] / med["dist_pred_to_gt"]
        res["note"] = "device events (numpy: wall clock, scaled from its subsample); medians of --reps after one warm-up round"
        print(json.dumps(res))


if __name__ == "__main__":
    main()
