#!/usr/bin/env python3
"""Time the finishing of the extracted mesh on the body-sized frame of tools/mesh_time.py, alternating in one process:
  clean    -- gpnerf_cube_clean (keep the largest solid component, fill the cavities) on the padded alpha cube;
  normals  -- gpnerf_mesh_normals at the cleaned mesh's vertices;
  cubes    -- gpnerf_mesh_count + gpnerf_mesh_emit on the same cube, for scale (it includes its host read of the two counts);
  host     -- the route there was before: cube.cpu(), scipy.ndimage.label twice (18-connectivity for the solid, 6 for the outside),
              np.where, and the copy back (wall clock, the device idle meanwhile).
clean, normals and cubes are device-event times.  Prints one JSON line: medians of --reps after one warm-up round, the stats, and
whether the host route's cube equals the device's bit for bit.  --device-only skips the host route (for the pass under
`rocprofv3 --kernel-trace --stats -- python tools/mesh_clean_time.py --device-only`, where the kernel times come from)."""
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
F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
L = importlib.import_module("gp-nerf_amd._lib")
syn = importlib.import_module("gp-nerf_amd.synthetic")


def host_route(cube, iso):
    """the cleaned cube by way of the host: (device tensor, seconds by stage)"""
    from scipy import ndimage
    t = [time.perf_counter()]
    c = cube.cpu().numpy()
    t.append(time.perf_counter())
    inside = ~(c < np.float32(iso))
    lab, n = ndimage.label(inside, structure=ndimage.generate_binary_structure(3, 2))
    if n:
        size = np.bincount(lab.reshape(-1), minlength=n + 1)
        size[0] = 0
        c = np.where(inside & (lab != int(np.argmax(size))), np.float32(0), c)      # (argmax: the first of the largest = the lowest label)
    t.append(time.perf_counter())
    lab, n = ndimage.label(c < np.float32(iso), structure=ndimage.generate_binary_structure(3, 1))
    if n:
        open_ = np.zeros(n + 1, dtype=bool)
        for ax in range(3):
            for side in (0, -1):
                open_[np.unique(np.take(lab, side, axis=ax))] = True
        open_[0] = True
        c = np.where(~open_[lab], np.float32(1), c)
    t.append(time.perf_counter())
    out = torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(cube.device)
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    d = np.diff(t)
    return out, {"copy_down": d[0], "label_solid": d[1], "label_outside": d[2], "copy_back": d[3], "total": float(d.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--device-only", action="store_true")
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
    cube, _ = F.density_lattice(fr, axes)
    iso = M.ISO_REFERENCE
    times = {"clean": [], "normals": [], "cubes": []}
    host = {}
    equal = None
    for rep in range(args.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        out, stats, _ = F.cube_clean(cube, iso, keep="largest", fill_cavities=True)
        e[1].record()
        verts, faces = F.marching_cubes(out, iso)
        e[2].record()
        normals = F.mesh_normals(out, verts, step=sc["voxel_size"])
        e[3].record()
        torch.cuda.synchronize()
        if not args.device_only:
            h_out, h = host_route(cube, iso)
            equal = bool(torch.equal(h_out.view(torch.int32), out.view(torch.int32)))
        if rep:
            times["clean"].append(e[0].elapsed_time(e[1]))
            times["cubes"].append(e[1].elapsed_time(e[2]))
            times["normals"].append(e[2].elapsed_time(e[3]))
            if not args.device_only:
                for k, v in h.items():
                    host.setdefault(k, []).append(v * 1e3)
    raw_v, raw_f = F.marching_cubes(cube, iso)
    points = int(cube.numel())
    ws = int(L.lib().gpnerf_cube_clean_workspace_bytes((__import__("ctypes").c_int32 * 3)(*cube.shape)))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"cube": list(cube.shape), "points": points, "stats": dict(zip(L.CUBE_STATS, stats.cpu().tolist())),
           "mesh_raw": [int(raw_v.shape[0]), int(raw_f.shape[0])], "mesh_clean": [int(verts.shape[0]), int(faces.shape[0])],
           "ms": med, "ms_min_max": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
           "points_per_s_clean": points / (med["clean"] * 1e-3),
           "workspace_bytes": ws, "workspace_bytes_per_point": ws / points,
           "resident_bytes": {"cube": 4 * points, "out_cube": 4 * points, "clean_workspace": ws, "marching_cubes_workspace": 8 * points}}
    if host:
        res["host_ms"] = {k: float(np.median(v)) for k, v in host.items()}
        res["host_equals_device"] = equal
        res["host_vs_device"] = res["host_ms"]["total"] / med["clean"]
    res["note"] = "device events (host: wall clock), alternating; medians of --reps after one warm-up round"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
