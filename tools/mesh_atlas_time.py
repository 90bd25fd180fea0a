#!/usr/bin/env python3
"""Time the per-face texture atlas (csrc/gpnerf_atlas.hip) on the body-sized golden mesh (tests/golden/mesh/mesh_body.npz: marching cubes
of its padded cube, index units) simplified by quadric clustering over cells of --cell lattice steps, on a ring of cameras that frame
the mesh at 512 x 512 (random images with four channels, the vertices' area-weighted normals, the grid built outside the timed region):
  atlas     -- frame.texture_atlas at --res texels per face edge from 3 and from 8 views, and its parts: texels (frame.atlas_texels),
               bake (frame.texture_points on the texel points), pack (frame.atlas_pack);
  shade     -- TextureAtlas.shade into 8 views over rasterize_mesh's face ids (the rasterisation itself is timed beside it);
  composed  -- the same results from torch ops, the baseline: the texel points by indexing the corners and broadcasting the weights,
               then frame.texture_points, the image by index_put_, and the draw by rasterize_mesh's interpolation of the barycentric
               weights plus gathers of the three taps.  Its results are compared with the kernels'.
Timing: device events around the wrapper, median (min - max) of --reps after a warm-up.  One JSON line per measurement, to stdout or
appended to --out.  Reads nothing outside the repository."""
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


def lattice(torch, R, dev):
    """(i, j) of a face's texels in index order, and their weights (wa, wb, wc) in float64, on the device"""
    ij = [(i, j) for j in range(R) for i in range(R - j)]
    i = torch.tensor([a for a, _ in ij], device=dev)
    j = torch.tensor([b for _, b in ij], device=dev)
    d = float(R - 1)
    return i, j, ((R - 1 - i - j).double() / d, i.double() / d, j.double() / d)


def composed_texels(torch, v, f, nrm, R):
    """atlas_texels from indexing and broadcasting: (points [T,3], normals [T,3]) float32"""
    _, _, (wa, wb, wc) = lattice(torch, R, v.device)
    fl = f.long()
    mix = lambda a: ((wa[None, :, None] * a[fl[:, 0]].double()[:, None] + wb[None, :, None] * a[fl[:, 1]].double()[:, None])
                     + wc[None, :, None] * a[fl[:, 2]].double()[:, None]).float().reshape(-1, a.shape[1]).contiguous()
    return mix(v), mix(nrm)


def composed_pack(torch, colors, n_faces, R, lay):
    """the image by index_put_ (no gutter fill: the composed draw does not read it either)"""
    i, j, _ = lattice(torch, R, colors.device)
    face = torch.arange(n_faces, device=colors.device)[:, None]
    odd = (face % 2) == 1
    x, y = torch.where(odd, R + 1 - i[None], i[None]), torch.where(odd, R - 1 - j[None], j[None])
    q = face // 2
    X, Y = (q % lay["cells_x"]) * (R + 2) + x, (q // lay["cells_x"]) * R + y
    image = torch.zeros((lay["height"], lay["width"], colors.shape[1]), device=colors.device)
    image.index_put_((Y.reshape(-1), X.reshape(-1)), colors)
    return image


def composed_shade(F, torch, image, v, f, Ks, RTs, H, W, R, lay):
    """the draw from rasterize_mesh plus gathers: the barycentric weights as interpolated attributes (each face's corners made its own
    vertices), then the SIMPLEX taps by indexing"""
    nf = int(f.shape[0])
    own_v = v[f.long().reshape(-1)].contiguous()
    own_f = torch.arange(3 * nf, device=v.device, dtype=torch.int32).reshape(nf, 3).contiguous()
    eye = torch.eye(3, device=v.device).repeat(nf, 1).contiguous()
    drawn = F.rasterize_mesh(own_v, own_f, Ks, RTs, H, W, want=("face_id",), attributes=eye)
    fid, u = drawn["face_id"].long(), drawn["image"].double()
    hit = fid >= 0
    fc = fid.clamp(min=0)
    top = float(R - 1)
    s = (u[..., 1] * top).clamp(0.0, top)
    t = torch.minimum((u[..., 2] * top).clamp(min=0.0), top - s)
    i0 = s.floor().long().clamp(max=R - 1)
    j0 = torch.minimum(t.floor().long(), R - 1 - i0)
    fs, ft = s - i0, t - j0
    lower = (fs + ft <= 1.0) | (i0 + j0 >= R - 2)
    w = [(1.0 - fs) - ft, torch.where(lower, fs, 1.0 - ft), torch.where(lower, ft, 1.0 - fs), (fs + ft) - 1.0]
    tap = [lower, torch.ones_like(lower), torch.ones_like(lower), ~lower]
    odd, q = (fc % 2) == 1, fc // 2
    num = torch.zeros(fid.shape + (image.shape[2],), device=v.device, dtype=torch.float64)
    den = torch.zeros(fid.shape, device=v.device, dtype=torch.float64)
    for k in range(4):
        i, j = i0 + (k & 1), j0 + (k >> 1)
        read = tap[k] & (i + j <= R - 1)
        ic, jc = torch.where(read, i, i0), torch.where(read, j, j0)
        x, y = torch.where(odd, R + 1 - ic, ic), torch.where(odd, R - 1 - jc, jc)
        col = image[(q // lay["cells_x"]) * R + y, (q % lay["cells_x"]) * (R + 2) + x].double()
        wk = torch.where(read, w[k], torch.zeros_like(w[k]))
        num += wk[..., None] * col
        den += wk
    return torch.where(hit[..., None], (num / den[..., None]).float(), torch.zeros((), device=v.device)), hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--res", type=int, default=8)
    ap.add_argument("--cell", type=float, default=2.0, help="the simplification's cell edge in lattice steps")
    ap.add_argument("--views", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    import raycast_cases as rc
    F = importlib.import_module("gp-nerf_amd.frame")
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "mesh", "mesh_body.npz"))
    cube = torch.from_numpy(np.ascontiguousarray(z["cube"], dtype=np.float32)).to(dev)
    mv, mf = F.marching_cubes(cube, float(z["iso"]))
    tv, tf = F.simplify_mesh(mv, mf, args.cell)[:2]
    tv, tf = tv.contiguous(), tf.contiguous()
    nrm = F.face_vertex_normals(tv, tf)
    grid = F.build_mesh_grid(tv, tf)
    v = tv.cpu().numpy()
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    centre, extent = 0.5 * (lo + hi), float((hi - lo).max())
    H = W = args.size
    R, nf = args.res, int(tf.shape[0])
    lay = F.atlas_layout(nf, R)

    def ring(V):
        cams = [rc.look_at(centre + 2.2 * extent * np.array([np.cos(a), np.sin(a), 0.3 * (-1) ** k]), centre, H, W, 1.9 * W)
                for k, a in enumerate(2 * np.pi * np.arange(V) / V + 0.1)]
        return np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    base = {"vertices": int(tv.shape[0]), "faces": nf, "marching_cubes_faces": int(mf.shape[0]), "cell": args.cell, "res": R,
            "texels": lay["n_texels"], "atlas": [lay["height"], lay["width"]], "image": [H, W, 4]}
    kept = {}
    for V in args.views:
        Ks, RTs = ring(V)
        images = torch.rand((V, H, W, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(V))
        res = {}

        def whole():
            res["atlas"] = F.texture_atlas(tv, tf, Ks, RTs, images, res=R, normals=nrm, grid=grid)

        def texels():
            res["tex"] = F.atlas_texels(tv, tf, R, normals=nrm)

        def bake():
            res["bake"] = F.texture_points(res["tex"]["points"], Ks, RTs, images, normals=res["tex"]["normals"], grid=grid)

        def pack():
            res["packed"] = F.atlas_pack(res["bake"]["color"], res["bake"]["views"], nf, R)

        def old_texels():
            res["old_tex"] = composed_texels(torch, tv, tf, nrm, R)

        def old_bake():
            res["old_bake"] = F.texture_points(res["old_tex"][0], Ks, RTs, images, normals=res["old_tex"][1], grid=grid)

        def old_pack():
            res["old_image"] = composed_pack(torch, res["old_bake"]["color"], nf, R, lay)

        def old_whole():
            old_texels(), old_bake(), old_pack()

        row = {"what": "atlas", "views": V, **base}
        for name, fn in (("atlas", whole), ("texels", texels), ("bake", bake), ("pack", pack), ("composed_atlas", old_whole),
                         ("composed_texels", old_texels), ("composed_bake", old_bake), ("composed_pack", old_pack)):
            row[f"{name}_ms_median_min_max"] = timed(fn, args.reps)
        cov = res["atlas"].coverage
        owned = (cov == 1) | (cov == 2)
        row["texel_points_differ_max"] = float((res["tex"]["points"] - res["old_tex"][0]).abs().max())
        row["image_differs_max_on_owned_texels"] = float((res["atlas"].image - res["old_image"])[owned].abs().max())
        row["composed_over_atlas"] = row["composed_atlas_ms_median_min_max"][0] / row["atlas_ms_median_min_max"][0]
        row["totals"] = [int(x) for x in res["atlas"].totals.cpu().numpy()]
        emit(row)
        kept[V] = res["atlas"]
    V = 8
    Ks, RTs = ring(V)
    atlas = kept.get(8) or next(iter(kept.values()))
    res = {}

    def raster():
        res["fid"] = F.rasterize_mesh(tv, tf, Ks, RTs, H, W, want=("face_id",))["face_id"]

    def shade():
        res["new"] = atlas.shade(res["fid"], tv, tf, Ks, RTs)

    def old_shade():
        res["old"] = composed_shade(F, torch, atlas.image, tv, tf, Ks, RTs, H, W, R, lay)

    row = {"what": "shade", "views": V, **base}
    for name, fn in (("rasterize", raster), ("shade", shade), ("composed_shade", old_shade)):
        row[f"{name}_ms_median_min_max"] = timed(fn, args.reps)
    hit = res["old"][1] & (res["fid"] >= 0)
    row["pixels_shaded"] = int((res["fid"] >= 0).sum())
    row["pixels_the_composed_draw_covers_alike"] = int(hit.sum())
    row["shade_differs_max"] = float((res["new"] - res["old"][0])[hit].abs().max())
    row["composed_over_shade"] = row["composed_shade_ms_median_min_max"][0] / row["shade_ms_median_min_max"][0]
    emit(row)
    return 0


if __name__ == "__main__":
    sys.exit(main())
