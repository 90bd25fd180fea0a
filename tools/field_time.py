#!/usr/bin/env python3
"""Time the field query (gpnerf_query_points) on the body-sized frame of tools/mesh_time.py with device events, alternating:
  query   -- rgb + sigma at the lattice points the occupancy keeps (world points, no cull);
  stage   -- gpnerf_project_gather + gpnerf_sample_volume + gpnerf_head_forward on the same points (the composition that was the
             nearest thing to a query before);
  colour  -- the colouring of the body mesh's vertices (lattice-index input, rgb), as Renderer(mesh_colors=True).render_mesh runs it.
Prints one JSON line: medians, points/s, and the work-done share of the fp32 MFMA peak.  The query's work done counts every
point's dense layers (bench.py's FLOP_PER_SAMPLE) minus the sigma feature layer of the 32-point tiles whose volume features are
all zero (ELU(bias) without the layer's MFMAs); the colouring's share is counted without that exit (an upper bound).
Kernel-by-kernel times come from a separate pass under `rocprofv3 --kernel-trace --stats -- python tools/field_time.py`."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
syn = importlib.import_module("gp-nerf_amd.synthetic")
FLOP_PER_POINT = 110848      # bench.py FLOP_PER_SAMPLE: 2 * MAC of NeRFHead.forward's dense layers, V = 3, C = 32
FLOP_SIGMA_LAYER = 16384     # ... of which sigmahead.out_geometry_fc (128 -> 64)
PEAK_TFLOPS = 157.3          # MI355X fp32 MFMA (bench.py's roofline peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=11)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sc = syn.make_scene(H=64, W=64, seed=args.seed, focal_mul=6.0, pose="random", body="capsules", bias_std=0.1, sigma_bias=0.5,
                        vol_relu=True)
    blob = F.pack_head(sc["head"], dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fr = F.Frame(t(sc["src_imgs"][0]), t(sc["featmaps"]), [t(v) for v in sc["volumes"]], t(sc["src_Ks"][0]), t(sc["src_poses"][0]),
                 sc["Rh"][0], sc["Th"][0], sc["bounds"][0, 0], sc["voxel_size"], sc["out_sh"][0], blob)
    fr.build_occupancy()
    box = F.mesh_box(fr, sc["voxel_size"], sc["bounds"][0, 0], sc["Rh"][0], sc["Th"][0])
    axes = F.lattice_axes(box, sc["voxel_size"])
    dims = tuple(len(a) for a in axes)
    # the kept lattice points, as tools/mesh_time.py selects them (grid coordinates with the demo's 0.005, occupancy > 0)
    ax = [torch.from_numpy(a).to(dev) for a in axes]
    pts = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    rays = torch.zeros((pts.shape[0], 8), device=dev)
    rays[:, :3] = pts
    saved = tuple(fr.c.voxel)
    for a in range(3):
        fr.c.voxel[a] = 0.005
    _, _, grid = F.sample_points(fr, rays, 1)
    for a in range(3):
        fr.c.voxel[a] = saved[a]
    del rays
    grid = grid.reshape(-1, 3)
    occ = TF.grid_sample(fr.occ[None, None], grid[None, None, None], align_corners=True, padding_mode="zeros").reshape(-1)
    kept = torch.nonzero(occ > 0).squeeze(1)
    kp, kg = pts.index_select(0, kept).contiguous(), grid.index_select(0, kept).contiguous()
    n = kp.shape[0]
    # the query's 32-point tiles whose 128 volume features are all zero in all 32 points (the sigma layer's exit); the stage
    # gather's taps are fused, but a feature is zero there exactly when it is zero in the query's multiply-then-add taps
    vol = F.sample_volume(fr, kg)
    nz = (vol != 0).any(1)
    nz = torch.cat([nz, torch.zeros(-n % 32, dtype=torch.bool, device=dev)]).reshape(-1, 32).any(1)
    empty_tiles = int((~nz).sum())
    del vol
    cube, _ = F.density_lattice(fr, axes)
    verts, faces = F.marching_cubes(cube, M.ISO_REFERENCE)
    lattice = F.lattice_of(axes, sc["voxel_size"])
    times = {"query": [], "stage_composition": [], "colour_vertices": []}
    for rep in range(args.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        F.query_points(fr, kp)
        e[1].record()
        feat, mask = F.project_gather(fr, kp)
        v = F.sample_volume(fr, kg)
        F.head_forward(blob, v, feat, mask)
        e[2].record()
        F.query_points(fr, verts, want=("rgb",), lattice=lattice)
        e[3].record()
        torch.cuda.synchronize()
        del feat, mask, v
        if rep:
            times["query"].append(e[0].elapsed_time(e[1]))
            times["stage_composition"].append(e[1].elapsed_time(e[2]))
            times["colour_vertices"].append(e[2].elapsed_time(e[3]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    nv = int(verts.shape[0])
    done = n * FLOP_PER_POINT - empty_tiles * 32 * FLOP_SIGMA_LAYER
    out = {"lattice": list(dims), "kept_points": n, "empty_space_tiles": empty_tiles, "tiles": (n + 31) // 32,
           "mesh_vertices": nv, "mesh_triangles": int(faces.shape[0]),
           "ms": med, "ms_min_max": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
           "points_per_s": {"query": n / (med["query"] * 1e-3), "stage_composition": n / (med["stage_composition"] * 1e-3),
                            "colour_vertices": nv / (med["colour_vertices"] * 1e-3)},
           "query_vs_stage": med["stage_composition"] / med["query"],
           "mfma_share": {"query": done / (med["query"] * 1e-3) / (PEAK_TFLOPS * 1e12),
                          "colour_vertices_upper_bound": nv * FLOP_PER_POINT / (med["colour_vertices"] * 1e-3) / (PEAK_TFLOPS * 1e12)},
           "note": "device events, alternating; medians of --reps after one warm-up round"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
