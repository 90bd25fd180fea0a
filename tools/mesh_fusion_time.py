#!/usr/bin/env python3
"""Time fusing depth maps into a truncated signed distance field (csrc/gpnerf_fusion.hip) on the body lattice of render_geometry: the
5 mm frame.dataset_lattice_axes lattice over the can_bounds of the body-sized golden frame (tests/golden/mesh/mesh_body.npz), 8 views at
512 x 512 (a ring of cameras that frame the box; the depth maps are frame.rasterize_mesh's of the golden mesh, made outside the timed
region), a band of 4 steps:
  oneshot   -- frame.fuse_depth: the counters' clear and the one-shot kernel, 4 bytes written per lattice point;
  integrate -- DepthFusion.integrate of the 8 views into a state that is there: 17 bytes in and 17 out per point;
  finalise  -- DepthFusion.grid: 17 bytes in, 4 out;
  reset     -- DepthFusion.reset: 17 bytes out;
  composed  -- the SAME computation from torch ops, the yardstick: per view the float64 projection of the (precomputed) lattice points,
               the nearest pixel gathered, the fates as masks, masked running sums, then the finalise as torch.where; its field is
               compared with the one-shot form's.
Timing: device events around the wrapper, median (min - max) of --reps after a warm-up.  Prints one JSON line per measurement and
appends it to --out (default profiles/r20/mesh_fusion_time.jsonl), with the ratio composed / oneshot and composed / (integrate +
finalise) and the achieved bytes per second against the state's traffic.  Reads nothing outside the repository."""
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


def composed(torch, pts, Ks, RTs, depth, band, z_near):
    """fuse_depth (no weights, carve) from torch ops: the field, float32 [n]"""
    n = pts.shape[0]
    V, H, W = depth.shape
    acc = torch.zeros((n,), device=pts.device, dtype=torch.float64)
    den = torch.zeros((n,), device=pts.device, dtype=torch.float64)
    hidden = torch.zeros((n,), device=pts.device, dtype=torch.bool)
    for v in range(V):
        c = pts @ RTs[v, :, :3].T + RTs[v, :, 3]
        h = c @ Ks[v].T
        z = h[:, 2]
        x, y = h[:, 0] / z, h[:, 1] / z
        ok = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(z) & (z >= z_near) & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        col = torch.round(x).clamp(0, W - 1).long()              # torch.round: half to even
        row = torch.round(y).clamp(0, H - 1).long()
        d = depth[v][row, col].double()
        valid = ok & (d > 0)
        background = torch.isinf(d)
        s = d - z
        hid = valid & ~background & (s < -band)
        add = valid & ~hid
        t = torch.where(background | (s >= band), torch.full_like(s, band), s)
        acc += torch.where(add, t, torch.zeros_like(t))
        den += add
        hidden |= hid
    mean = (acc / den).float().clamp(-band, band)
    return torch.where(den > 0, mean, torch.where(hidden, -band, band).float())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--band-steps", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "mesh_fusion_time.jsonl"))
    args = ap.parse_args()
    import torch
    import texture_cases as tc
    from golden_cases import load, scene_of
    F = importlib.import_module("gp-nerf_amd.frame")
    L = importlib.import_module("gp-nerf_amd._lib")
    dev = torch.device("cuda:0")
    z, meta = load("mesh/mesh_body")
    vs = [float(x) for x in scene_of(meta)["voxel_size"]]
    box = np.asarray(z["can_bounds"], np.float32)
    axes = F.dataset_lattice_axes(box, vs)
    lo, dims = [float(a[0]) for a in axes], tuple(len(a) for a in axes)
    n = int(np.prod(dims))
    band = float(np.float32(args.band_steps * max(vs)))
    # the golden mesh (index units of its padded cube) laid into the box, as the surface the views see
    cube = torch.from_numpy(np.ascontiguousarray(z["cube"], dtype=np.float32)).to(dev)
    tv, tf = F.marching_cubes(cube, float(z["iso"]))
    span = (tv.max(dim=0).values - tv.min(dim=0).values).cpu().numpy().astype(np.float64)
    scale = float(((box[1] - box[0]).astype(np.float64) / span).min()) * 0.9
    centre = 0.5 * (box[0] + box[1]).astype(np.float64)
    mid = 0.5 * (tv.max(dim=0).values + tv.min(dim=0).values).double()
    world = ((tv.double() - mid) * scale + torch.from_numpy(centre).to(dev)).float().contiguous()
    H = W = args.size
    V = args.views
    size = float(np.linalg.norm(box[1] - box[0]))
    Ks, RTs = tc.ring_cameras(V, H, W, focal=W * 2.5 / 1.15, distance=2.5 * size, target=tuple(centre))
    depth = F.rasterize_mesh(world, tf, Ks, RTs, H, W, want=("depth",))["depth"]
    res = {}

    def oneshot():
        res["one"] = F.fuse_depth(depth, Ks, RTs, lo, vs, dims, band)

    fusion = F.DepthFusion(lo, vs, dims, band, dev)
    one_ms = timed(oneshot, args.reps)
    int_ms = timed(lambda: fusion.integrate(depth, Ks, RTs), args.reps)
    fin_ms = timed(lambda: res.__setitem__("grid", fusion.grid()), args.reps)
    reset_ms = timed(fusion.reset, args.reps)
    fusion.integrate(depth, Ks, RTs)
    state_values = fusion.grid().values
    pts = torch.stack(torch.meshgrid(*[torch.from_numpy(a).to(dev) for a in axes], indexing="ij"), dim=-1).reshape(-1, 3).double()
    Kt, RTt = torch.from_numpy(Ks).to(dev), torch.from_numpy(RTs).to(dev)

    def old():
        res["old"] = composed(torch, pts, Kt, RTt, depth, band, 1e-6)

    old_ms = timed(old, args.reps)
    one = res["one"].values.reshape(-1)
    differ = one != res["old"]
    gbs = lambda nbytes, ms: nbytes * n / (ms * 1e-3) / 1e9
    line = {"what": "fusion", "lattice": list(dims), "points": n, "views": V, "image": [H, W], "band": band,
            "oneshot_ms_median_min_max": one_ms, "integrate_ms_median_min_max": int_ms, "finalise_ms_median_min_max": fin_ms,
            "reset_ms_median_min_max": reset_ms, "composed_ms_median_min_max": old_ms,
            "composed_over_oneshot": old_ms[0] / one_ms[0], "composed_over_integrate_plus_finalise": old_ms[0] / (int_ms[0] + fin_ms[0]),
            "oneshot_GBps_of_4_bytes_per_point": gbs(4, one_ms[0]), "integrate_GBps_of_34_bytes_per_point": gbs(34, int_ms[0]),
            "finalise_GBps_of_21_bytes_per_point": gbs(21, fin_ms[0]), "reset_GBps_of_17_bytes_per_point": gbs(17, reset_ms[0]),
            "depth_map_bytes": int(depth.numel() * 4),
            "fates": {name: [int(x) for x in res["one"].fusion_stats.cpu().numpy()[:, k]] for k, name in enumerate(L.FUSION_FATES)},
            "totals": dict(zip(L.FUSION_TOTALS, [int(x) for x in res["one"].fusion_totals.cpu().numpy()])),
            "state_form_equals_oneshot": bool(torch.equal(state_values.reshape(-1), one)),
            "points_where_the_composed_field_differs": int(differ.sum().item()),
            "composed_difference_max": float((one - res["old"]).abs().max().item())}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
