#!/usr/bin/env python3
"""Time ray casting against a mesh (csrc/gpnerf_raycast.hip) on the body-sized golden mesh (tests/golden/mesh/mesh_body.npz: 79 948
faces, marching cubes of its padded cube, index units) along the 512 x 512 pixel rays of one hull-style camera that frames it:
  grid      -- raycast_mesh through the mesh's grid at the default mesh_grid_caps and at two other cell_caps (a quarter and four
               times the default), nearest and any mode; the grid is built outside the timed region;
  brute     -- the brute-force form on a --brute-rays crop of the same frame, bit-compared with the grid form there;
  raster    -- rasterize_mesh for the same camera, the share of pixels at which the two name the same face, and the largest depth
               difference there;
  work      -- cells visited and faces tested per ray, counted on the host by the restatement of THE WALK (tests/raycast_cases.py)
               over --count-rays rays of the frame and the device grid's own header: once with the result known from the start (the
               fewest cells the early stop can leave) and once without any stop (the most);
  registers -- VGPRs, scratch and LDS of the kernels from the compiler's resource remarks for the product's flags.
Timing: device events around the wrapper, median (min - max) of --reps after a warm-up.  Prints one JSON line per measurement.
Reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import re
import subprocess
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


def resources():
    """{kernel: {vgprs, scratch_bytes_per_lane, lds_bytes, occupancy}} from hipcc's kernel-resource-usage remarks"""
    csrc = os.path.join(ROOT, "gp-nerf_amd", "csrc")
    flags = "-O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -Wall -Wno-unused-function -Inodiag".split()
    try:
        r = subprocess.run(["hipcc"] + flags + ["--cuda-device-only", "-c", "-o", os.devnull, "gpnerf_raycast.hip",
                                                "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True, timeout=300)
    except Exception as err:
        return {"error": repr(err)}
    out, name = {}, None
    for line in r.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", m.group(1))
            name = re.match(r"[a-z_]+", name).group(0) + ("<any>" if "ILb1E" in m.group(1) else "<nearest>" if "ILb0E" in m.group(1) else "")
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out or {"error": r.stderr[-400:]}


def walk_counts(rays, t_known, header, vertices, faces):
    """cells and entries (faces tested, with repeats) per ray by the host restatement of THE WALK over the device grid's header"""
    import raycast_cases as rc
    n = np.asarray(header["cells"], np.int64)
    lo, inv = header["lo"], header["inv"]
    tri = vertices[faces]
    c0 = np.stack([rc.cell_of(tri.min(axis=1)[:, k], lo[k], inv[k], n[k]) for k in range(3)], axis=1)
    c1 = np.stack([rc.cell_of(tri.max(axis=1)[:, k], lo[k], inv[k], n[k]) for k in range(3)], axis=1)
    count = np.zeros(int(n.prod()), np.int64)
    for a, b in zip(c0, c1):
        ix = np.ix_(range(a[0], b[0] + 1), range(a[1], b[1] + 1), range(a[2], b[2] + 1))
        count.reshape(n)[ix] += 1
    grid = {"lo": lo, "size": header["size"], "inv": inv, "n": n, "span": (c1 - c0).max(axis=0)}
    res = {}
    for label, known in (("stop_known_from_the_start", True), ("no_stop", False)):
        cells = entries = 0
        for ray, t in zip(rays, t_known):
            r = ray.copy()
            if known and np.isfinite(t):
                r[7] = t
            visited = rc.walk_cells(r, grid)
            cells += len(visited)
            entries += int(count[visited].sum()) if visited else 0
        res[label] = {"cells_per_ray": cells / len(rays), "faces_tested_per_ray": entries / len(rays)}
    res["span"] = [int(s) for s in grid["span"]]
    res["entries_per_occupied_cell"] = float(count[count > 0].mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--brute-rays", type=int, default=16384)
    ap.add_argument("--count-rays", type=int, default=1500)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    import torch
    import raycast_cases as rc
    F = importlib.import_module("gp-nerf_amd.frame")
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "mesh", "mesh_body.npz"))
    cube = torch.from_numpy(np.ascontiguousarray(z["cube"], dtype=np.float32)).to(dev)
    tv, tf = F.marching_cubes(cube, float(z["iso"]))
    v, f = tv.cpu().numpy(), tf.cpu().numpy()
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    centre, extent = 0.5 * (lo + hi), float((hi - lo).max())
    H = W = args.size
    K, RT = rc.look_at(centre + np.array([2.2, 0.6, 0.4]) * extent, centre, H, W, 1.9 * W)
    Ks, RTs = K[None], RT[None]
    rays = F.pixel_rays(Ks, RTs, H, W)
    torch.cuda.synchronize()
    nf, n_rays = int(tf.shape[0]), H * W
    d_cell, _ = F.mesh_grid_caps(nf)
    base = {"faces": nf, "vertices": int(tv.shape[0]), "rays": n_rays, "image": [H, W]}
    print(json.dumps(dict(base, what="pixel_rays", ms_median_min_max=timed(lambda: F.pixel_rays(Ks, RTs, H, W), args.reps))), flush=True)
    default = None
    for cell_cap in (d_cell // 4, d_cell, 4 * d_cell):
        grid = F.build_mesh_grid(tv, tf, cell_cap=cell_cap)
        header = grid.header()
        res = {}

        def call(mode="nearest"):
            res[mode] = F.raycast_mesh(rays, grid=grid, mode=mode)

        near_ms, any_ms = timed(call, args.reps), timed(lambda: call("any"), args.reps)
        t = res["nearest"]["t"]
        row = dict(base, what="grid", cell_cap=cell_cap, cells=header["cells"], entries=header["needed"], nearest_ms_median_min_max=near_ms,
                   any_ms_median_min_max=any_ms, rays_hit=int(torch.isfinite(t).sum()), mrays_per_s=n_rays / near_ms[0] / 1e3,
                   build_ms_median_min_max=timed(lambda: F.build_mesh_grid(tv, tf, cell_cap=cell_cap, check=False), args.reps))
        if cell_cap == d_cell:
            default = (grid, res["nearest"], near_ms)
            pick = np.random.default_rng(0).choice(n_rays, args.count_rays, replace=False)
            row["work_counted_on_the_host"] = walk_counts(rays.reshape(-1, 8)[pick].cpu().numpy(), t.reshape(-1)[pick].cpu().numpy(), header, v, f)
        print(json.dumps(row), flush=True)
    grid, near, near_ms = default
    # the brute-force form on a crop of the frame's middle rows
    rows = max(1, args.brute_rays // W)
    r0 = (H - rows) // 2
    crop = rays[0, r0:r0 + rows].reshape(-1, 8).contiguous()
    out = {}

    def brute():
        out["res"] = F.raycast_mesh(crop, tv, tf)

    brute_ms = timed(brute, max(3, args.reps // 2))
    same = bool(torch.equal(out["res"]["t"].view(torch.int32), near["t"][0, r0:r0 + rows].reshape(-1).view(torch.int32)) and
                torch.equal(out["res"]["face"], near["face"][0, r0:r0 + rows].reshape(-1)))
    grid_crop_ms = timed(lambda: F.raycast_mesh(crop, grid=grid), args.reps)
    print(json.dumps(dict(base, what="brute", rays=int(crop.shape[0]), brute_ms_median_min_max=brute_ms, grid_same_rays_ms_median_min_max=grid_crop_ms,
                          brute_over_grid=brute_ms[0] / grid_crop_ms[0], bit_equal_to_the_grid_form=same)), flush=True)
    # the rasteriser for the same camera
    drawn = {}

    def draw():
        drawn.update(F.rasterize_mesh(tv, tf, Ks, RTs, H, W))

    raster_ms = timed(draw, args.reps)
    covered = drawn["face_id"] >= 0
    hit = near["face"] >= 0
    same_face = covered & (drawn["face_id"] == near["face"])
    diff = (drawn["depth"] - near["t"]).abs()[same_face]
    print(json.dumps(dict(base, what="raster", rasterize_ms_median_min_max=raster_ms, grid_over_raster=near_ms[0] / raster_ms[0],
                          pixels_covered=int(covered.sum()), rays_hit=int(hit.sum()), coverage_agrees_share=float((covered == hit).float().mean()),
                          same_face_share_of_covered=float(same_face.sum() / covered.sum()),
                          depth_difference_max_where_same_face=float(diff.max()), depth_difference_mean_where_same_face=float(diff.mean()))), flush=True)
    if not args.no_resources:
        print(json.dumps({"what": "registers", "kernels": resources()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
