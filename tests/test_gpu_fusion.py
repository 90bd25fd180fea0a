"""GPU: fusing depth maps into a truncated signed distance field (gpnerf_fusion.hip).  Values, flags, stats and totals against the numpy
float64 restatement of include/gpnerf_hip.h's THE DEFINITION (tests/fusion_cases.py) -- bit for bit, one-shot and state forms; every
comparison at its edge; chunked integration, reset and graph replay changing no bit; the closed loop through the rasteriser; the signs
beside mesh_sdf; Renderer.render_fusion end to end.  Lattices of at most 40 x 40 x 33 points, images of at most 48 x 48 (64 x 64
for the renderer)."""
import importlib
import os
import sys
import types
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import fusion_cases as fc
import texture_cases as tc

pytestmark = pytest.mark.gpu
F = importlib.import_module("gp-nerf_amd.frame")
L = importlib.import_module("gp-nerf_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def args_of(case, views=None, use_weights=True, **kw):
    """(depth, Ks, RTs, weights) on the device / host and the keywords of a case cut to `views`"""
    sel = list(range(len(case["depth"]))) if views is None else list(views)
    w = case.get("weights") if use_weights else None
    opts = dict(z_near=case.get("z_near", 1e-6), carve=case.get("carve", True))
    opts.update(kw)
    return dev(case["depth"][sel]), case["Ks"][sel], case["RTs"][sel], None if w is None else dev(w[sel]), opts


def oneshot(case, views=None, use_weights=True, **kw):
    d, Ks, RTs, w, opts = args_of(case, views, use_weights, **kw)
    g = F.fuse_depth(d, Ks, RTs, case["lo"], case["step"], case["dims"], case["band"], weights=w, want_flags=True, **opts)
    return {"values": g.values, "flags": g.flags, "stats": g.fusion_stats, "totals": g.fusion_totals}


def stateful(case, chunks=None, use_weights=True, fusion=None, **kw):
    fusion = fusion if fusion is not None else F.DepthFusion(case["lo"], case["step"], case["dims"], case["band"], DEV)
    stats = []
    for ch in (chunks if chunks is not None else [range(len(case["depth"]))]):
        d, Ks, RTs, w, opts = args_of(case, ch, use_weights, **kw)
        stats.append(fusion.integrate(d, Ks, RTs, weights=w, **opts))
    g = fusion.grid()
    return {"values": g.values, "flags": fusion.flags, "stats": torch.cat(stats), "totals": g.stats, "sum": fusion.sum, "weight": fusion.weight}


def assert_same(got, ref, what, keys=("stats", "totals", "flags", "values")):
    torch.cuda.synchronize()
    for k in keys:
        a, b = bits(got[k]), bits(ref[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert not len(bad), (what, k, f"{len(bad)} of {a.size} differ", bad[:5].tolist())


# ---- 1. bit equality with the restatement

@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("use_weights", [True, False])
def test_both_forms_equal_the_restatement_bit_for_bit(carve, use_weights):
    case = fc.general_case()
    ref = fc.run_case(case, carve=carve, **({} if use_weights else {"weights": None}))
    print(f"carve={carve} weights={use_weights}: dims {case['dims']}, 8 views; pairs per fate", dict(zip(fc.FATES, ref["stats"].sum(axis=0).tolist())),
          "totals", dict(zip(fc.TOTALS, ref["totals"].tolist())))
    assert (ref["stats"].sum(axis=0) >= 1).all(), "the case reaches every fate"
    assert_same(oneshot(case, use_weights=use_weights, carve=carve), ref, "one-shot")
    assert_same(stateful(case, use_weights=use_weights, carve=carve), ref, "state", keys=("stats", "totals", "flags", "values", "sum", "weight"))


@pytest.mark.parametrize("dims", [(12, 10, 1), (12, 10, 63), (12, 10, 64), (12, 10, 65), (1, 17, 33), (13, 1, 9), (40, 40, 33)])
@pytest.mark.parametrize("views", [1, 8])
def test_lattice_sizes_around_a_wavefront_and_view_counts(dims, views):
    case = fc.general_case(dims=dims)
    sel = range(views)
    ref = fc.run_case(dict(case, depth=case["depth"][:views], weights=case["weights"][:views], Ks=case["Ks"][:views], RTs=case["RTs"][:views]))
    assert (ref["stats"].sum(axis=1) == int(np.prod(dims))).all()
    assert_same(oneshot(case, views=sel), ref, ("one-shot", dims, views))
    assert_same(stateful(case, chunks=[sel]), ref, ("state", dims, views), keys=("stats", "totals", "flags", "values", "sum", "weight"))


def test_one_pixel_images():
    """1 x 1, 1 x 7 and 7 x 1 images: the frame is a point or a segment, and the pixel index stays inside it"""
    for H, W in ((1, 1), (1, 7), (7, 1)):
        K = np.array([[4.0, 0, (W - 1) / 2], [0, 4.0, (H - 1) / 2], [0, 0, 1.0]])
        depth = (1.0 + 0.03125 * np.arange(H * W, dtype=np.float32)).reshape(1, H, W)
        case = {"Ks": K[None], "RTs": fc.EXACT_RT[None], "depth": depth, "lo": np.array([-0.75, -0.75, 0.75]), "step": np.array([0.125, 0.125, 0.0625]),
                "dims": (13, 13, 9), "band": 0.25}
        ref = fc.run_case(case)
        assert ref["stats"][0, fc.NEAR] >= 1 and ref["stats"][0, fc.OUTSIDE] >= 1
        assert_same(oneshot(case), ref, (H, W))


# ---- 2. every comparison at its edge

@pytest.mark.parametrize("name", sorted(fc.boundary_cases()))
def test_every_comparison_at_its_edge(name):
    case = fc.boundary_cases()[name]
    ref = fc.run_case(case)
    assert np.array_equal(ref["fate"], case["expect"])
    for got in (oneshot(case), stateful(case), stateful(case, chunks=[[v] for v in range(len(case["depth"]))])):
        assert_same(got, ref, name)
        # a view's row of stats IS the fate of its pairs: one lattice point per fate listed
        want = np.stack([np.bincount(case["expect"][:, v], minlength=6) for v in range(case["expect"].shape[1])])
        assert np.array_equal(got["stats"].cpu().numpy(), want), name
        if "values" in case:
            assert np.array_equal(bits(got["values"]), bits(case["values"])), "a half pixel goes to the even column / row"


# ---- 3. chunking, one-shot, reset

def test_chunks_the_one_shot_form_and_reset_leave_the_same_bits():
    case = fc.general_case(dims=(23, 19, 33))
    keys = ("stats", "totals", "flags", "values", "sum", "weight")
    whole = stateful(case)
    assert_same(whole, fc.run_case(case), "whole", keys=keys)
    halves = stateful(case, chunks=[range(0, 4), range(4, 8)])
    singles = stateful(case, chunks=[[v] for v in range(8)])
    host = {k: whole[k].cpu().numpy() for k in keys}
    assert_same(halves, host, "0..3 then 4..7", keys=keys)
    assert_same(singles, host, "one view at a time", keys=keys)
    assert_same(oneshot(case), host, "one-shot == integrate + finalise")
    used = F.DepthFusion(case["lo"], case["step"], case["dims"], case["band"], DEV)
    stateful(dict(case, depth=case["depth"][::-1].copy()), fusion=used)
    assert used.weight.abs().sum().item() > 0
    used.reset()
    assert not used.sum.any().item() and not used.weight.any().item() and not used.flags.any().item()
    assert_same(stateful(case, fusion=used), host, "reset() then integrate == a fresh object", keys=keys)
    more = stateful(case, chunks=[range(8), range(8)])         # 16 views: the same eight twice
    ref16 = fc.run_case(case, chunks=[range(8), range(8)])
    assert_same(more, ref16, "16 views", keys=keys)


# ---- 4. determinism

def test_two_runs_and_two_graph_replays_change_no_bit():
    case = fc.general_case(dims=(23, 19, 33))
    base = {k: v.cpu().numpy() for k, v in oneshot(case).items()}
    assert_same(oneshot(case), base, "second run")
    d, Ks, RTs, w, opts = args_of(case)
    fusion = F.DepthFusion(case["lo"], case["step"], case["dims"], case["band"], DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one = F.fuse_depth(d, Ks, RTs, case["lo"], case["step"], case["dims"], case["band"], weights=w, want_flags=True, **opts)
        fusion.reset()
        st = fusion.integrate(d, Ks, RTs, weights=w, **opts)
        grid = fusion.grid()
    for _ in range(2):
        for t in (one.values, one.flags, one.fusion_stats, one.fusion_totals, st, grid.values, grid.stats, fusion.sum, fusion.weight, fusion.flags):
            t.fill_(7)
        g.replay()
        assert_same({"values": one.values, "flags": one.flags, "stats": one.fusion_stats, "totals": one.fusion_totals}, base, "graph replay, one-shot")
        assert_same({"values": grid.values, "flags": fusion.flags, "stats": st, "totals": grid.stats}, base, "graph replay, state")


# ---- 5. closed loops

def test_the_icosphere_through_the_rasteriser_and_back():
    m = fc.convex_case()
    v, f = dev(m["vertices"]), dev(m["faces"])
    depth = F.rasterize_mesh(v, f, m["Ks"], m["RTs"], m["H"], m["W"], want=("depth",))["depth"]
    grid = F.fuse_depth(depth, m["Ks"], m["RTs"], m["lo"], m["step"], m["dims"], m["band"], want_flags=True)
    ref = fc.run_case(dict(m, depth=depth.cpu().numpy()))
    assert_same({"values": grid.values, "flags": grid.flags, "stats": grid.fusion_stats, "totals": grid.fusion_totals}, ref, "closed loop")
    assert ref["stats"][:, fc.OUTSIDE].sum() == 0 and ref["totals"][1] > 0
    fv, ff = grid.offset_mesh(0.0)
    assert fv.shape[0] > 500 and ff.shape[0] > 1000
    res = F.read_mesh_metrics(F.mesh_metrics((fv, ff), (v, f), n_samples=20000))
    radius = fv.to(torch.float64).norm(dim=1)
    print(f"icosphere(3), 6 axis views 48 x 48, step {m['step'][0]}, band {m['band']}: fused mesh {fv.shape[0]} vertices, {ff.shape[0]} faces; "
          f"accuracy {res['accuracy']:.5f} completeness {res['completeness']:.5f} chamfer {res['chamfer']:.5f} normal consistency "
          f"{res['normal_consistency']:.4f}; vertex radius {radius.min().item():.4f} .. {radius.max().item():.4f}; "
          f"totals {dict(zip(fc.TOTALS, ref['totals'].tolist()))}")
    # the host test's derived bound, on the device's field: a vertex of the zero set lies on a crossing edge, within one step + the
    # sign's slack (under the margin) of the polyhedron, which lies between the spheres of radius r_in and 1
    assert (radius - 1.0).abs().max().item() < float(m["step"][0]) + m["margin"] + (1.0 - m["r_in"])


def test_two_squares_hidden_from_one_side_emptied_from_another():
    s = fc.squares_case()
    v, f = dev(s["vertices"]), dev(s["faces"])
    depth = F.rasterize_mesh(v, f, s["Ks"], s["RTs"], s["H"], s["W"], want=("depth",))["depth"]
    n = int(np.prod(s["dims"]))
    band = np.float32(s["band"])
    front = F.fuse_depth(depth[:1].contiguous(), s["Ks"][:1], s["RTs"][:1], s["lo"], s["step"], s["dims"], s["band"], want_flags=True)
    assert front.fusion_stats.cpu().tolist() == [[0, 0, 0, 0, n, 0]], "every lattice point between the squares is HIDDEN"
    assert front.fusion_totals.cpu().tolist() == [0, 0, n, 0] and (front.values == -band).all().item() and (front.flags == 1).all().item()
    both = F.fuse_depth(depth, s["Ks"], s["RTs"], s["lo"], s["step"], s["dims"], s["band"], want_flags=True)
    assert both.fusion_stats.cpu().tolist() == [[0, 0, 0, 0, n, 0], [0, 0, 0, n, 0, 0]], "the side view sees past them: EMPTY"
    assert both.fusion_totals.cpu().tolist() == [n, 0, 0, 0] and (both.values == band).all().item() and (both.flags == 1).all().item()
    ref = fc.run_case(dict(s, depth=depth.cpu().numpy()))
    assert_same({"values": both.values, "flags": both.flags, "stats": both.fusion_stats, "totals": both.fusion_totals}, ref, "squares")
    blind = F.fuse_depth(depth[1:].contiguous(), s["Ks"][1:], s["RTs"][1:], s["lo"], s["step"], s["dims"], s["band"], carve=False)
    assert blind.fusion_totals.cpu().tolist() == [0, 0, 0, n] and (blind.values == band).all().item(), "without carving the side view says nothing"


# ---- 6. beside mesh_sdf

def test_the_signs_are_mesh_sdfs_beyond_the_margin():
    """icosphere(3), convex, in six axis views that cover the lattice.  margin = the pixel footprint at the farthest lattice depth + one
    lattice step (tests/test_fusion_host.py derives why the sign is decided beyond it and checks the restatement alone): wherever
    |mesh_sdf| exceeds it, the fused field has mesh_sdf's sign; the points left out stay under the case's cap."""
    m = fc.convex_case()
    v, f = dev(m["vertices"]), dev(m["faces"])
    depth = F.rasterize_mesh(v, f, m["Ks"], m["RTs"], m["H"], m["W"], want=("depth",))["depth"]
    fused = F.fuse_depth(depth, m["Ks"], m["RTs"], m["lo"], m["step"], m["dims"], m["band"]).values
    sdf = F.mesh_sdf(v, f, m["lo"], m["step"], m["dims"], band=0.5, rule="nonzero").values
    assert 0.5 > m["margin"]
    far = sdf.abs() > m["margin"]
    n, compared = sdf.numel(), int(far.sum().item())
    print(f"beside mesh_sdf: margin {m['margin']:.4f} (footprint {m['footprint']:.4f} + step {m['step'][0]}), {compared} of {n} points compared, "
          f"{1 - compared / n:.3f} left out (cap {m['cap']:.3f}); inside {int((sdf[far] < 0).sum().item())}, outside {int((sdf[far] > 0).sum().item())}")
    assert 1 - compared / n < m["cap"]
    assert (sdf[far] < 0).sum().item() > 1000 and (sdf[far] > 0).sum().item() > 5000
    assert ((fused[far] < 0) == (sdf[far] < 0)).all().item() and (fused[far] != 0).all().item()


# ---- 7. Renderer.render_fusion

@pytest.fixture(scope="module")
def fusion_renderer():
    """test_gpu_hull.py's renderer on the mesh_body golden frame, with eight ring cameras at 64 x 64 around the box as hull cameras"""
    from golden_cases import load, scene_of
    z, meta = load("mesh/mesh_body")
    sc = scene_of(meta)
    p = os.path.join(ROOT, "gp-nerf_amd", "plugins")
    if p not in sys.path:
        sys.path.insert(0, p)
    m = types.ModuleType("fixed_encoder")

    class Enc(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("tests pass featmaps in the batch")

    m.build_encoder = lambda cfg: Enc()
    sys.modules["fixed_encoder"] = m
    hip_render = importlib.import_module("hip_render")
    cfg = NS(encoder=NS(file="fixed_encoder", name="resnet34", out_ch=32),
             head=NS(file="hip_head", rgb=NS(use_rgbhead=False), sigma=NS(code_dim=32, n_heads=4, n_layers=4, n_smpl=6890, outdims=[32, 32, 32, 32])),
             dataset=NS(train=NS(name="zju_mocap", chunk=400), test=NS(name="zju_mocap", chunk=2000), voxel_size=[float(x) for x in sc["voxel_size"]]),
             train=NS(n_rays=1024, n_samples=32), test=NS(mesh_th=50, test_seq="s"))
    r = hip_render.build_render(cfg).to(DEV).eval()
    sd = r.state_dict()
    for k, v in sc["head"].items():
        sd["nerfhead." + k] = torch.from_numpy(v.copy())
    r.load_state_dict(sd, strict=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    base = {k: t(sc[k]) for k in ("src_imgs", "src_Ks", "src_poses", "feature", "coord", "out_sh", "bounds", "Rh", "R", "Th")}
    base["featmaps"] = t(sc["featmaps"])
    base["volumes"] = [t(v) for v in sc["volumes"]]
    box = np.asarray(z["can_bounds"], np.float32)
    centre, size = 0.5 * (box[0] + box[1]).astype(np.float64), float(np.linalg.norm(box[1] - box[0]))
    Ks, RTs = tc.ring_cameras(8, 64, 64, focal=64 * 2.5 * size / (1.15 * size), distance=2.5 * size, target=tuple(centre))
    batch = dict(base, hull_masks=torch.ones((1, 8, 64, 64), device=DEV, dtype=torch.uint8), hull_Ks=t(Ks)[None], hull_RTs=t(RTs)[None],
                 can_bounds=t(box)[None])
    return NS(r=r, batch=batch, Ks=Ks, RTs=RTs, box=box, vs=[float(x) for x in sc["voxel_size"]])


def test_render_fusion_is_fuse_depth_on_its_own_depth_maps(fusion_renderer):
    fr = fusion_renderer
    with torch.no_grad():
        out = fr.r.render_fusion(fr.batch)
    assert set(out) == {"mesh", "sdf", "depth_maps", "fusion_stats", "time_slots", "etime", "rtime"}
    depth, sdf = out["depth_maps"], out["sdf"]
    assert tuple(depth.shape) == (8, 64, 64) and depth.dtype == torch.float32
    seen = torch.isfinite(depth)
    print(f"render_fusion: {seen.float().mean().item():.3f} of the pixels carry a depth")
    assert seen.any().item() and (~seen).any().item() and (depth[seen] > 0).all().item() and torch.isposinf(depth[~seen]).all().item()
    axes = F.dataset_lattice_axes(fr.box, fr.vs)
    assert sdf.dims == tuple(len(a) for a in axes) and abs(sdf.band - 4 * max(fr.vs)) < 1e-6
    direct = F.fuse_depth(depth, fr.Ks, fr.RTs, [float(a[0]) for a in axes], fr.vs, sdf.dims, sdf.band)
    torch.cuda.synchronize()
    assert np.array_equal(bits(sdf.values), bits(direct.values)), "sdf.values == fuse_depth on the returned depth maps"
    assert sdf.stats.cpu().tolist() == direct.fusion_totals.cpu().tolist()
    fs = out["fusion_stats"]
    assert fs["seen"] + fs["interior"] + fs["unknown"] == int(np.prod(sdf.dims)) and len(fs["per_view"]["near"]) == 8 and fs["surface"] > 0
    v, f = sdf.offset_mesh(0.0)
    assert np.array_equal(out["mesh"].vertices, v.cpu().numpy()) and np.array_equal(out["mesh"].faces, f.cpu().numpy())
    assert len(out["mesh"].faces) > 100
    lo, hi = fr.box[0] - 0.02, fr.box[1] + 0.02
    assert (out["mesh"].vertices >= lo).all() and (out["mesh"].vertices <= hi).all(), "the mesh lives in the WORLD frame, inside can_bounds"
    # render_geometry's mesh of the same frame: index units of the padded cube -> world
    with torch.no_grad():
        geo = fr.r.render_geometry(fr.batch)
    gv = np.stack([axes[a].astype(np.float64)[0] + (geo["mesh"].vertices[:, a].astype(np.float64) - F.MESH_PAD) * fr.vs[a] for a in range(3)],
                  axis=1).astype(np.float32)
    res = F.read_mesh_metrics(F.mesh_metrics((v, f), (dev(gv), dev(geo["mesh"].faces.astype(np.int32))), n_samples=20000))
    print(f"render_fusion on mesh_body, 8 ring views 64 x 64: lattice {sdf.dims}, band {sdf.band:.4f}; fused mesh {len(out['mesh'].vertices)} vertices "
          f"{len(out['mesh'].faces)} faces, render_geometry's {len(gv)} / {len(geo['mesh'].faces)}; chamfer {res['chamfer']:.5f} (accuracy "
          f"{res['accuracy']:.5f}, completeness {res['completeness']:.5f}); totals "
          f"{ {k: fs[k] for k in fc.TOTALS} }; time_slots {out['time_slots']}")


def test_render_fusion_names_the_missing_keys(fusion_renderer):
    fr = fusion_renderer
    batch = {k: v for k, v in fr.batch.items() if k not in ("hull_RTs", "can_bounds")}
    with pytest.raises(L.GpnerfError, match="'hull_masks', 'hull_Ks', 'hull_RTs', 'can_bounds'.*missing: 'hull_RTs', 'can_bounds'"):
        fr.r.render_fusion(batch)
    bad = dict(fr.batch, hull_Ks=fr.batch["hull_Ks"] * 2.0)
    with pytest.raises(L.GpnerfError, match="last row"):
        fr.r.render_fusion(bad)
