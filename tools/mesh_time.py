#!/usr/bin/env python3
"""Time the geometry mode (Renderer.render_mesh's device work) on a body-sized frame with device events, and the stage entry points
(gpnerf_project_gather + gpnerf_sample_volume + gpnerf_head_forward) on the same kept points, alternating.  Prints one JSON line.

The lattice kernel's work-done share of the fp32 MFMA peak counts 38 656 FLOP per lane of every 32-point tile with a kept point
(the sigma feature layer 128 -> 64 and the density branch 134 -> 64 -> 32 -> 16: the layers the kernel runs on the matrix pipe).
Kernel-by-kernel times come from a separate pass under `rocprofv3 --kernel-trace --stats -- python tools/mesh_time.py`; the kernels
are density_lattice_kernel, mc_count_kernel, mc_scan_blocks_kernel and mc_emit_kernel."""
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
FLOP_PER_POINT = 2 * (128 * 64 + 134 * 64 + 64 * 32 + 32 * 16)
PEAK_TFLOPS = 157.3          # MI355X fp32 MFMA (bench.py's roofline peak)
LAT_BY, LAT_BZ = 4, 8


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
    # the kept points for the stage composition: grid coordinates from gpnerf_sample_points (zero-length rays, the demo's 0.005),
    # occupancy > 0 (a non-negative volume: the decision does not depend on the summation order)
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
    grid = grid.reshape(-1, 3)
    occ = TF.grid_sample(fr.occ[None, None], grid[None, None, None], align_corners=True, padding_mode="zeros").reshape(-1)
    kept = torch.nonzero(occ > 0).squeeze(1)
    kp, kg = pts.index_select(0, kept).contiguous(), grid.index_select(0, kept).contiguous()
    # tiles of the padded cube that hold a kept point (the ones that run the matrix work)
    keep = np.zeros(tuple(d + 2 * F.MESH_PAD for d in dims), bool)
    keep[F.MESH_PAD:-F.MESH_PAD, F.MESH_PAD:-F.MESH_PAD, F.MESH_PAD:-F.MESH_PAD] = (occ > 0).cpu().numpy().reshape(dims)
    PX, PY, PZ = keep.shape
    kb = np.pad(keep, ((0, 0), (0, -PY % LAT_BY), (0, -PZ % LAT_BZ)))
    busy_tiles = int(kb.reshape(PX, kb.shape[1] // LAT_BY, LAT_BY, kb.shape[2] // LAT_BZ, LAT_BZ).any(axis=(2, 4)).sum())
    times = {"lattice": [], "marching_cubes": [], "stage_composition": []}
    for rep in range(args.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        cube, n_kept = F.density_lattice(fr, axes)
        e[1].record()
        e[2].record()
        v, f = F.marching_cubes(cube, M.ISO_REFERENCE)        # (its count read synchronises inside)
        e[3].record()
        feat, mask = F.project_gather(fr, kp)
        vol = F.sample_volume(fr, kg)
        F.head_forward(blob, vol, feat, mask)
        e[4].record()
        torch.cuda.synchronize()
        if rep:
            times["lattice"].append(e[0].elapsed_time(e[1]))
            times["marching_cubes"].append(e[2].elapsed_time(e[3]))
            times["stage_composition"].append(e[3].elapsed_time(e[4]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    pad_pts = int(np.prod(keep.shape))
    out = {"lattice": list(dims), "padded_points": pad_pts, "kept": int(n_kept.item()), "tiles_with_kept": busy_tiles,
           "vertices": int(v.shape[0]), "triangles": int(f.shape[0]),
           "ms": med, "ms_min_max": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
           "lattice_vs_stage": med["stage_composition"] / med["lattice"],
           "lattice_mfma_share": busy_tiles * 32 * FLOP_PER_POINT / (med["lattice"] * 1e-3) / (PEAK_TFLOPS * 1e12),
           "resident_mb": {"cube": pad_pts * 4 / 2 ** 20, "mesh_workspace": pad_pts * 8 / 2 ** 20},
           "note": "device events; marching_cubes includes the count read between its two launches; stage_composition on the kept points"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
