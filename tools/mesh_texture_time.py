#!/usr/bin/env python3
"""Time colouring a mesh from calibrated views (csrc/gpnerf_texture.hip) on the body-sized golden mesh (tests/golden/mesh/mesh_body.npz:
marching cubes of its padded cube, index units): its vertices against itself, from 3 and from 8 synthetic views at 512 x 512 (a ring of
cameras that frame the mesh, random images with four channels, the faces' area-weighted normals, the grid built outside the timed
region):
  texture      -- frame.texture_points with the mesh's grid: prepare, the ANY cast over all n x views rows, blend;
  composed     -- the same result from what there was before: frame.mesh_visibility over all n x views pairs, and in torch the float64
                  projection, the facing test and weights, F.grid_sample(align_corners=True) per view and the blend; the colours of
                  the two are compared;
  no_occlusion -- frame.texture_points without a mesh: prepare and blend alone, so texture - no_occlusion is what the separate cast
                  launch (and writing its rows) costs.
Timing: device events around the wrapper, median (min - max) of --reps after a warm-up.  Prints one JSON line per measurement, with the
ratio composed / texture and the share of the pairs that reached the cast.  Reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def composed(F, torch, pts, nrm, Ks, RTs, eyes, images_nchw, grid, cos_min, sharpness, z_near):
    """texture_points' blend from mesh_visibility, torch arithmetic and grid_sample: (colour [n,C], views-used mask [n,V])"""
    n, V = pts.shape[0], Ks.shape[0]
    H, W = images_nchw.shape[2:]
    seen = F.mesh_visibility(pts, eyes, grid=grid).bool()
    p, nr = pts.double(), nrm.double()
    num = torch.zeros((n, images_nchw.shape[1]), device=pts.device, dtype=torch.float64)
    den = torch.zeros((n,), device=pts.device, dtype=torch.float64)
    used = torch.zeros((n, V), device=pts.device, dtype=torch.bool)
    for v in range(V):
        c = p @ RTs[v, :, :3].T + RTs[v, :, 3]
        h = c @ Ks[v].T
        x, y, z = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2], h[:, 2]
        ok = torch.isfinite(x) & torch.isfinite(y) & (z >= z_near) & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        d = (eyes[v][None] - pts).double()
        a, nn, vv = (nr * d).sum(1), (nr * nr).sum(1), (d * d).sum(1)
        ok &= (a > 0) & (a * a >= cos_min * cos_min * nn * vv) & seen[:, v]
        w = ((a * a) / (nn * vv)) ** sharpness
        g = torch.stack([2 * x / max(W - 1, 1) - 1, 2 * y / max(H - 1, 1) - 1], dim=1).float().reshape(1, n, 1, 2)
        col = torch.nn.functional.grid_sample(images_nchw[v:v + 1], g, mode="bilinear", padding_mode="border", align_corners=True)[0, :, :, 0].T
        w = torch.where(ok, w, torch.zeros_like(w))
        num += w[:, None] * col.double()
        den += w
        used[:, v] = ok
    return (num / den[:, None]).float(), used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--views", type=int, nargs="+", default=[3, 8])
    args = ap.parse_args()
    import torch
    import raycast_cases as rc
    F = importlib.import_module("gp-nerf_amd.frame")
    L = importlib.import_module("gp-nerf_amd._lib")
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "mesh", "mesh_body.npz"))
    cube = torch.from_numpy(np.ascontiguousarray(z["cube"], dtype=np.float32)).to(dev)
    tv, tf = F.marching_cubes(cube, float(z["iso"]))
    nrm = F.face_vertex_normals(tv, tf)
    grid = F.build_mesh_grid(tv, tf)
    v = tv.cpu().numpy()
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    centre, extent = 0.5 * (lo + hi), float((hi - lo).max())
    H = W = args.size
    n = int(tv.shape[0])
    cos_min, sharpness, z_near = 0.2, 2, 1e-6
    for V in args.views:
        cams = [rc.look_at(centre + 2.2 * extent * np.array([np.cos(a), np.sin(a), 0.3 * (-1) ** k]), centre, H, W, 1.9 * W)
                for k, a in enumerate(2 * np.pi * np.arange(V) / V + 0.1)]
        Ks, RTs = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
        images = torch.rand((V, H, W, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(V))
        res = {}

        def new(occlude=True):
            res["new" if occlude else "free"] = F.texture_points(tv, Ks, RTs, images, normals=nrm, grid=grid if occlude else None, cos_min=cos_min,
                                                                 sharpness=sharpness, z_near=z_near)

        new_ms, free_ms = timed(new, args.reps), timed(lambda: new(False), args.reps)
        eyes = torch.from_numpy(np.stack([-(RT[:, :3].T @ RT[:, 3]) for RT in RTs]).astype(np.float32)).to(dev)
        Kt, RTt = torch.from_numpy(Ks).to(dev), torch.from_numpy(RTs).to(dev)
        nchw = images.permute(0, 3, 1, 2).contiguous()

        def old():
            res["old"] = composed(F, torch, tv, nrm, Kt, RTt, eyes, nchw, grid, cos_min, sharpness, z_near)

        old_ms = timed(old, args.reps)
        stats = res["new"]["stats"].cpu().numpy()
        bits = (res["new"]["views"][:, None].int() >> torch.arange(V, device=dev)[None]) & 1
        same = bits.bool() == res["old"][1]
        both = same.all(dim=1) & (res["new"]["views"] != 0)
        diff = float((res["new"]["color"][both] - res["old"][0][both]).abs().max())
        reached = int(stats[:, L.TEXTURE_USED].sum() + stats[:, L.TEXTURE_OCCLUDED].sum())
        print(json.dumps({"what": "texture", "vertices": n, "faces": int(tf.shape[0]), "views": V, "image": [H, W, 4],
                          "texture_ms_median_min_max": new_ms, "composed_ms_median_min_max": old_ms, "no_occlusion_ms_median_min_max": free_ms,
                          "composed_over_texture": old_ms[0] / new_ms[0], "cast_share_of_texture": max(0.0, 1.0 - free_ms[0] / new_ms[0]),
                          "pairs": n * V, "pairs_reaching_the_cast": reached, "share_reaching_the_cast": reached / (n * V),
                          "fates": {name: [int(x) for x in stats[:, k]] for k, name in enumerate(L.TEXTURE_STATS)},
                          "totals": [int(x) for x in res["new"]["totals"].cpu().numpy()],
                          "pairs_the_composed_route_decides_alike": float(same.float().mean()),
                          "colour_difference_max_where_alike": diff}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
