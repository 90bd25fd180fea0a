#!/usr/bin/env python3
"""Time the dense renderer's geometry mode on the person-shaped frame of DESIGN 4.5 (device events, routes alternating in one process,
medians of --reps).  Prints one JSON line.

  (i)  gpnerf_visual_hull against the host restatement of ZjumocapDataset.prepare_inside_pts (tests/hull_cases.py: the reference's
       route, numpy on a loader worker; timed once with the host clock) on the same 5 mm lattice and four 1024 x 1024 masks;
  (ii) gpnerf_density_lattice_masked against the composition available without it: torch.nonzero of the hull (a host read for the
       count), a 12 B/point list, gpnerf_query_points (density only, alpha), a scatter into the cube, the padding.

The hull's cameras stand on a ring around the body's long axis; the masks are ellipses (1) with a border band (100), so that the
kept share is a body's.  Kernel times come from a separate pass under `rocprofv3 --kernel-trace --stats -- python tools/hull_time.py`;
the kernels are visual_hull_kernel, density_lattice_kernel<true> and field_points_kernel<false>."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hull_cases as hc  # noqa: E402

F = importlib.import_module("gp-nerf_amd.frame")
syn = importlib.import_module("gp-nerf_amd.synthetic")


def ring(box, n, size, focal, dist):
    centre = 0.5 * (box[0] + box[1]).astype(np.float64)
    ext = (box[1] - box[0]).astype(np.float64)
    up = np.eye(3)[int(np.argmax(ext))]
    a, b = np.eye(3)[(int(np.argmax(ext)) + 1) % 3], np.eye(3)[(int(np.argmax(ext)) + 2) % 3]
    Ks, RTs = [], []
    for i in range(n):
        th = 0.3 + i * np.pi / n
        eye = centre + dist * (np.cos(th) * a + np.sin(th) * b) + 0.2 * up
        z = centre - eye
        z /= np.linalg.norm(z)
        x = np.cross(z, up + 0.03 * a)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        RTs.append(np.concatenate([R, (-R @ eye)[:, None]], axis=1))
        Ks.append(np.array([[focal, 0.0, size / 2 - 0.37], [0.0, focal * 1.01, size / 2 + 0.21], [0.0, 0.0, 1.0]]))
    return np.stack(Ks), np.stack(RTs)


def ellipse(size, ry, rx, band):
    yy, xx = np.mgrid[:size, :size].astype(np.float64)
    c = size / 2
    m = np.zeros((size, size), np.uint8)
    m[((yy - c) / (ry + band)) ** 2 + ((xx - c) / (rx + band)) ** 2 <= 1] = 100
    m[((yy - c) / ry) ** 2 + ((xx - c) / rx) ** 2 <= 1] = 1
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement (a profiler pass)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sc = syn.make_scene(H=64, W=64, seed=args.seed, focal_mul=6.0, pose="random", body="capsules", bias_std=0.1, sigma_bias=0.5,
                        vol_relu=True)
    blob = F.pack_head(sc["head"], dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fr = F.Frame(t(sc["src_imgs"][0]), t(sc["featmaps"]), [t(v) for v in sc["volumes"]], t(sc["src_Ks"][0]), t(sc["src_poses"][0]),
                 sc["Rh"][0], sc["Th"][0], sc["bounds"][0, 0], sc["voxel_size"], sc["out_sh"][0], blob)
    box = F.mesh_box(fr, sc["voxel_size"], sc["bounds"][0, 0], sc["Rh"][0], sc["Th"][0])
    fr.c.occ, fr.occ = None, None                       # (the box needed it; the masked lattice must not)
    axes = F.dataset_lattice_axes(box, [float(v) for v in sc["voxel_size"]])
    dims = tuple(len(a) for a in axes)
    size = 1024
    long_px = 0.5 * float((box[1] - box[0]).max()) * 620.0 / 3.0
    Ks, RTs = ring(box, 4, size, 620.0, 3.0)
    masks_np = np.stack([ellipse(size, 0.8 * long_px, 0.22 * long_px * (1 + 0.1 * i), 8) for i in range(4)])
    masks = t(masks_np)
    ax = [t(a) for a in axes]
    pad = F.MESH_PAD
    times = {"hull": [], "masked_lattice": [], "composition": []}
    for rep in range(args.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        inside, n_inside = F.visual_hull(axes, masks, Ks, RTs)
        e[1].record()
        cube, n_kept = F.density_lattice(fr, axes, inside=inside)
        e[2].record()
        idx = torch.nonzero(inside)                                                   # the count read
        pts = torch.stack([ax[0][idx[:, 0]], ax[1][idx[:, 1]], ax[2][idx[:, 2]]], dim=1).contiguous()
        alpha = F.query_points(fr, pts, want=("sigma", "alpha"))["alpha"]
        inner = torch.zeros(dims, device=dev)
        inner[idx[:, 0], idx[:, 1], idx[:, 2]] = alpha
        cube2 = TF.pad(inner, (pad,) * 6)
        e[3].record()
        torch.cuda.synchronize()
        if rep:
            for k, i in (("hull", 0), ("masked_lattice", 1), ("composition", 2)):
                times[k].append(e[i].elapsed_time(e[i + 1]))
    same = bool(torch.equal(cube.view(torch.int32), cube2.view(torch.int32)))
    med = {k: float(np.median(v)) for k, v in times.items()}
    host_s, host_equal = None, None
    if not args.no_host:
        t0 = time.time()
        ref, tie, _ = hc.hull_np(axes, masks_np, hc.cams_of(Ks, RTs))
        host_s = time.time() - t0
        got = inside.cpu().numpy()
        host_equal = bool(((got == ref) | tie).all()) and int(tie.sum()) <= hc.TIE_CAP * tie.size
    n_pts = int(np.prod(dims))
    # the lattice kernel's tiles (4 x 8 bricks of the padded cube's x-slices) that hold a kept point run all 32 lanes' matrix work;
    # the composition's list is compact: ceil(n / 32) tiles, all full
    keep = np.zeros(tuple(d + 2 * pad for d in dims), bool)
    keep[pad:-pad, pad:-pad, pad:-pad] = inside.cpu().numpy() != 0
    PX, PY, PZ = keep.shape
    kb = np.pad(keep, ((0, 0), (0, -PY % 4), (0, -PZ % 8)))
    busy = int(kb.reshape(PX, kb.shape[1] // 4, 4, kb.shape[2] // 8, 8).any(axis=(2, 4)).sum())
    all_tiles = PX * (kb.shape[1] // 4) * (kb.shape[2] // 8)
    out = {"lattice": list(dims), "points": n_pts, "n_inside": int(n_inside.item()), "n_kept": int(n_kept.item()),
           "tiles": {"lattice_all": all_tiles, "lattice_with_kept": busy, "composition": (int(n_kept.item()) + 31) // 32},
           "ms": med, "ms_min_max": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
           "hull_store_gbps": n_pts / (med["hull"] * 1e-3) / 1e9, "hull_host_restatement_s": host_s, "hull_equals_host_restatement": host_equal,
           "composition_vs_masked": med["composition"] / med["masked_lattice"], "composition_equals_masked_bits": same,
           "loader_bytes_saved": {"pts": n_pts * 12, "inside": n_pts},
           "note": "device events, medians; the composition includes torch.nonzero's host read; the host restatement is numpy, one run"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
