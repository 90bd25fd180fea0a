#!/usr/bin/env python3
"""Generate the geometry-mode vectors tests/golden/mesh/*.npz by RUNNING the reference's inference renderer with a head built with
use_rgbhead=False: libs/renders/demo_render.py Renderer.render -> batchify_rays -> render_rays (:96-376), the box (:166-175), the
torch.range lattice (:249-263), the occupancy cull (:270-283), Projector.compute, NeRFSigmaHead.test_forward, rgbhead.out_geometry_fc,
the alpha cube and its padding (:366-371).

The stand-ins are make_golden.py's (spconv, the encoder, the device-name shim; imported from it, that file is unchanged), plus
`mcubes.marching_cubes`, stubbed to capture (cube, iso) -- mcubes is not installed -- and `trimesh.Trimesh`, an inert holder.
Captured besides the cube: the three lattice axes and can_bounds (the torch.range / torch.stack calls of render_rays), the kept set
(the single-channel F.grid_sample of the occupancy volume, > 0) and its size.  Inputs are regenerated from (seed, config) by
gp-nerf_amd/synthetic.py; each .npz carries a SHA-256 over the input bytes.
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

MESH_CASES = [
    # a person-shaped frame (capsule-limbed vertices, pyramid-shaped sparse levels), the box scaled down to keep the fixture small
    ("mesh_body", dict(H=64, W=64, seed=71, focal_mul=1.2, body="capsules", aabb_half=(0.14, 0.22, 0.07), voxel=0.005,
                       sigma_bias=-3, bias_std=0.1, pose="random")),
    # trained-like parameters (trained_h1_s64's distributions): head x 1 with biases, density bias -10, feature maps and levels x 4 with log-normal tails
    ("mesh_trained", dict(H=64, W=64, seed=72, focal_mul=1.5, aabb_half=(0.12, 0.16, 0.05), voxel=0.005, vol_occupancy=0.4,
                          sigma_bias=-10.0, head_scale=1.0, feat_scale=4.0, feat_tail=0.5, vol_scale=4.0, bias_std=0.3, pose="random")),
]
ISO = 1 / 50.0


def run_mesh_case(name, scene_kw, neg_ray=False):
    syn = importlib.import_module("gp-nerf_amd.synthetic")
    demo = importlib.import_module("demo_render")
    trainhead = importlib.import_module("trainhead")
    scene = syn.make_scene(**scene_kw)
    head = trainhead.NeRFHead(in_feat_ch=32, n_smpl=6890, code_dim=32, attn_n_heads=4,
                              spconv_n_layers=4, spconv_out_dim=[32, 32, 32, 32], use_rgbhead=False)
    sd = head.state_dict()
    for k, v in scene["head"].items():
        sd[k] = torch.from_numpy(v.copy())
    head.load_state_dict(sd, strict=True)
    net = [mg._Pass()]
    for v in scene["volumes"]:
        net += [mg._Pass(), mg._Level(torch.from_numpy(v))]
    head.sigmahead.xyzc_net.net = nn.ModuleList(net)
    enc = mg._FixedEncoder(torch.from_numpy(scene["featmaps"]))
    r = demo.Renderer(enc, head, is_train=False, neg_ray_train=neg_ray, neg_ray_val=neg_ray, n_rays=1024, n_samples=32,
                      voxel_size=[float(x) for x in scene["voxel_size"]], chunk=400)
    r.eval()
    batch = mg.to_batch(scene)
    batch["target_K_inv"] = torch.from_numpy(scene["target_K_inv"].copy())
    cap = {"axes": [], "boxes": []}
    mc = sys.modules["mcubes"]
    mc.marching_cubes = lambda cube, iso: (cap.update(cube=np.array(cube, copy=True), iso=float(iso)) or
                                           (np.zeros((0, 3)), np.zeros((0, 3), np.int64)))
    sys.modules["trimesh"].Trimesh = lambda v, f: types.SimpleNamespace(vertices=v, faces=f)
    orig_range, orig_stack, orig_gs = torch.range, torch.stack, TF.grid_sample

    def rng(*a, **k):
        out = orig_range(*a, **k)
        cap["axes"].append(out.numpy().astype(np.float32).copy())
        return out

    def stack(ts, *a, **k):
        out = orig_stack(ts, *a, **k)
        if len(ts) == 2 and all(t.dim() == 1 and t.shape[0] == 3 for t in ts):
            cap["boxes"].append(out.numpy().astype(np.float32).copy())          # can_bounds (:175)
        return out

    def grid_sample(inp, grid, *a, **k):
        out = orig_gs(inp, grid, *a, **k)
        if inp.shape[1] == 1:                                                   # masks3d, the cull (:274-281)
            cap["keep"] = (out.reshape(-1) > 0).numpy().copy()
        return out

    torch.range, torch.stack, TF.grid_sample = rng, stack, grid_sample
    try:
        with torch.no_grad(), mg._device_shim():
            ret = r.render(batch)
    finally:
        torch.range, torch.stack, TF.grid_sample = orig_range, orig_stack, orig_gs
    assert "mesh" in ret and cap["iso"] == ISO, sorted(ret)
    cube, axes, keep = cap["cube"].astype(np.float32), cap["axes"], cap["keep"]
    assert len(axes) == 3 and len(cap["boxes"]) == 1
    X, Y, Z = (len(a) for a in axes)
    assert cube.shape == (X + 20, Y + 20, Z + 20) and keep.shape == (X * Y * Z,)
    assert (cube > ISO).any() and (cube < ISO).any(), "the cube must have values on both sides of the iso value"
    assert not cube.reshape(-1)[np.pad(np.zeros((X, Y, Z), bool), 10, constant_values=True).reshape(-1)].any()
    out = {"cube": cube, "axis_x": axes[0], "axis_y": axes[1], "axis_z": axes[2], "can_bounds": cap["boxes"][0],
           "keep_bits": np.packbits(keep), "n_kept": np.int64(keep.sum()), "iso": np.float32(cap["iso"])}
    meta = {"scene_kw": scene_kw, "neg_ray": bool(neg_ray), "sha256_inputs": mg.sha_inputs(scene), "torch": torch.__version__,
            "numpy": np.__version__, "reference": "libs/renders/demo_render.py Renderer.render with use_rgbhead=False, eval, CPU fp32 "
            "via the device-name shim; mcubes.marching_cubes captured"}
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    # (a directory of their own: the dense-renderer parity tests take every *.npz directly under tests/golden/ for theirs)
    os.makedirs(os.path.join(HERE, "mesh"), exist_ok=True)
    path = os.path.join(HERE, "mesh", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: lattice {X}x{Y}x{Z}, kept {int(keep.sum())}, alpha max {cube.max():.3f}, "
          f"{int((cube > ISO).sum())} above iso -> {os.path.getsize(path)} B")


def main():
    mg._install_stubs()
    mg._paths()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    only = set(sys.argv[1:])
    for name, kw in MESH_CASES:
        if not only or name in only:
            run_mesh_case(name, kw)


if __name__ == "__main__":
    main()
