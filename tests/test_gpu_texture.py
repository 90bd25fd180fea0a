"""GPU: colouring points from calibrated views (gpnerf_texture.hip).  color, weight, views, stats and totals against the numpy float64
restatement of include/gpnerf_hip.h's THE DEFINITION (tests/texture_cases.py) -- bit for bit; the sphere's closed loop through the
rasteriser; occlusion deciding a colour; agreement with mesh_visibility pair by pair; the invariances (face order, grid against brute
force, graph replay, outputs singly); the pixel convention against the per-ray path's gather; Renderer(mesh_texture="views") and
MeshEvaluator(texture=True) end to end.  At most 841 points, 8 views and 1 280 faces per case."""
import importlib

import numpy as np
import pytest
import torch

import texture_cases as tc

pytestmark = pytest.mark.gpu
F = importlib.import_module("gp-nerf_amd.frame")
L = importlib.import_module("gp-nerf_amd._lib")
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)


def host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run(case, n=None, views=None, form="grid", use_normals=True, use_masks=True, use_mesh=True, use_fallback=True, channels=None, **kw):
    """(device result on the host, restatement) of a texture_cases case cut to n points, `views` views and `channels` channels"""
    n = len(case["points"]) if n is None else n
    V = len(case["Ks"]) if views is None else views
    C = case["images"].shape[-1] if channels is None else channels
    images = np.ascontiguousarray(np.resize(case["images"][:V], (V,) + case["images"].shape[1:3] + (C,))) if C != case["images"].shape[-1] \
        else case["images"][:V]
    args = dict(normals=case["normals"][:n] if use_normals and case.get("normals") is not None else None,
                masks=case["masks"][:V] if use_masks and case.get("masks") is not None else None,
                fallback=np.ascontiguousarray(np.resize(case["fallback"][:n], (n, C))) if use_fallback and case.get("fallback") is not None else None)
    if "z_near" in case:
        kw.setdefault("z_near", case["z_near"])
    mesh = (case["vertices"], case["faces"]) if use_mesh and case.get("faces") is not None else (None, None)
    ref = tc.restate(case["points"][:n], case["Ks"][:V], case["RTs"][:V], images, vertices=mesh[0], faces=mesh[1], **args, **kw)
    dkw = {k: dev(v) for k, v in args.items()}
    if mesh[0] is not None:
        v, f = dev(mesh[0]), dev(mesh[1])
        dkw.update(dict(grid=F.build_mesh_grid(v, f)) if form == "grid" else dict(vertices=v, faces=f))
    got = host(F.texture_points(dev(case["points"][:n]), case["Ks"][:V], case["RTs"][:V], dev(images), **dkw, **kw))
    return got, ref


def assert_same(got, ref, what):
    for k in ("views", "stats", "totals", "color", "weight"):
        bad = np.flatnonzero((bits(got[k]) != bits(ref[k])).reshape(len(ref[k]), -1).any(axis=1))
        assert not len(bad), (what, k, bad[:5].tolist(), got[k][bad[:5]].tolist(), ref[k][bad[:5]].tolist())


# ---- 1. bit equality with the restatement

@pytest.mark.parametrize("mode", ["blend", "best"])
@pytest.mark.parametrize("sharpness", [0, 1, 4])
def test_every_output_equals_the_restatement_bit_for_bit(mode, sharpness):
    case = tc.general_case()
    got, ref = run(case, mode=mode, sharpness=sharpness)
    print(f"{mode} k={sharpness}: {len(case['points'])} points, 8 views; fates", dict(zip(tc.FATES, ref["stats"].sum(axis=0).tolist())),
          "totals", ref["totals"].tolist())
    assert_same(got, ref, (mode, sharpness))
    assert (got["stats"].sum(axis=1) == len(case["points"])).all() and got["totals"].sum() == len(case["points"])
    assert set(np.unique(ref["fate"])) == set(range(6)), "the case reaches every fate"


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("views", [1, 8])
def test_channels_views_and_the_optional_inputs(channels, views):
    case = tc.general_case()
    for use_normals, use_masks, use_mesh, use_fallback in ((True, True, True, True), (False, True, True, False), (True, False, False, True),
                                                           (False, False, False, False)):
        for mode in ("blend", "best"):
            got, ref = run(case, views=views, channels=channels, use_normals=use_normals, use_masks=use_masks, use_mesh=use_mesh,
                           use_fallback=use_fallback, mode=mode, background=[0.25, 0.5, 0.75, 1.0][:channels])
            assert_same(got, ref, (channels, views, use_normals, use_masks, use_mesh, use_fallback, mode))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_point_counts_around_a_wavefront(n):
    case = tc.general_case(n=n)
    for form in ("grid", "brute"):
        got, ref = run(case, form=form)
        assert_same(got, ref, (n, form))
    none = F.texture_points(torch.empty((0, 3), device=DEV), case["Ks"], case["RTs"], dev(case["images"]))
    assert none["color"].shape == (0, 3) and host(none)["stats"].tolist() == [[0] * 6] * 8 and host(none)["totals"].tolist() == [0, 0]


def test_one_pixel_wide_and_one_pixel_high_images():
    rng = np.random.default_rng(8)
    for H, W in ((1, 7), (7, 1), (1, 1)):
        K = np.array([[4.0, 0, (W - 1) / 2], [0, 4.0, (H - 1) / 2], [0, 0, 1.0]])
        RT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
        pts = np.zeros((40, 3), np.float32)
        pts[:, 0] = rng.uniform(-1, 1, 40) * (W > 1)
        pts[:, 1] = rng.uniform(-1, 1, 40) * (H > 1)
        pts[:, 2] = 1.0
        case = {"points": pts, "Ks": K[None], "RTs": RT[None], "images": tc.random_images(1, H, W, 4, 9)}
        got, ref = run(case)
        assert_same(got, ref, (H, W))
        assert ref["stats"][0, tc.USED] >= 10 and (H * W > 1) == (ref["stats"][0, tc.OUTSIDE] > 0)


def test_the_frame_is_inclusive_and_the_near_plane_exact():
    e = tc.exact_case()
    case = dict(e, images=tc.random_images(1, e["H"], e["W"], 3, 4))
    got, ref = run(case, sharpness=0)
    assert_same(got, ref, "exact")
    assert np.array_equal(ref["fate"][:, 0], e["expect"]) and np.array_equal(got["views"], (e["expect"] == tc.USED).astype(np.uint8))
    assert np.array_equal(got["color"][10], case["images"][0, 8, 8])


# ---- 2. the sphere's closed loop

@pytest.fixture(scope="module")
def sphere():
    s = tc.sphere_case()
    v, f, col = dev(s["vertices"]), dev(s["faces"]), dev(s["colours"])
    drawn = F.rasterize_mesh(v, f, s["Ks"], s["RTs"], s["H"], s["W"], want=(), attributes=col)["image"]
    return dict(s, v=v, f=f, images=drawn, images_host=drawn.cpu().numpy())


def test_the_sphere_is_coloured_back_from_its_own_pictures(sphere):
    s = sphere
    got = host(F.texture_mesh(s["v"], s["f"], s["Ks"], s["RTs"], s["images"], normals=dev(s["normals"]), cos_min=s["cos_min"]))
    ref = tc.restate(s["vertices"], s["Ks"], s["RTs"], s["images_host"], normals=s["normals"], cos_min=s["cos_min"], vertices=s["vertices"],
                     faces=s["faces"])
    assert_same(got, ref, "sphere")
    st = got["stats"]
    assert ((st[:, tc.USED] + st[:, tc.BACKFACING]) == 642).all() and (st[:, tc.OCCLUDED] == 0).all() and got["totals"].tolist() == [642, 0]
    assert st[:, tc.USED].tolist() == [161] * 6
    err = float(np.abs(got["color"].astype(np.float64) - s["colours"]).max())
    err64 = float(np.abs(ref["color"].astype(np.float64) - s["colours"]).max())
    ref32 = tc.restate(s["vertices"], s["Ks"], s["RTs"], s["images_host"], normals=s["normals"], cos_min=s["cos_min"], dtype=np.float32)
    d32 = float(np.abs(ref32["color"].astype(np.float64) - ref["color"].astype(np.float64)).max())
    print(f"sphere closed loop: colour error against the vertex colours: device {err:.3e}, float64 restatement {err64:.3e}; "
          f"float32 variant against float64 {d32:.3e}")
    assert err <= err64 + 4 * d32
    own = host(F.texture_mesh(s["v"], s["f"], s["Ks"], s["RTs"], s["images"], cos_min=s["cos_min"]))     # the faces' own normals
    assert own["totals"].tolist() == [642, 0] and (own["stats"][:, tc.OCCLUDED] == 0).all()


# ---- 3. occlusion decides

def test_occlusion_decides_the_colour():
    q = tc.squares_case()
    v, f = dev(q["vertices"]), dev(q["faces"])
    image = F.rasterize_mesh(v, f, q["K"][None], q["RT"][None], q["H"], q["W"], want=(), attributes=dev(q["colours"]))["image"]
    pts, sh = dev(q["points"]), q["shadowed"]
    nrm = dev(np.tile(np.float32([0, 0, 1]), (len(sh), 1)))
    fallback = np.full((len(sh), 3), 0.125, np.float32)
    assert sh.sum() >= 100 and (~sh).sum() >= 100
    for kw in (dict(grid=F.build_mesh_grid(v, f)), dict(vertices=v, faces=f)):
        got = host(F.texture_points(pts, q["K"][None], q["RT"][None], image, normals=nrm, fallback=dev(fallback), **kw))
        assert np.array_equal(got["views"], (~sh).astype(np.uint8))
        assert got["stats"][0].tolist() == [int((~sh).sum()), 0, 0, 0, 0, int(sh.sum())]
        assert np.array_equal(got["color"][sh], fallback[sh]) and (got["color"][~sh] == q["back"]).all()
    blind = host(F.texture_points(pts, q["K"][None], q["RT"][None], image, normals=nrm, fallback=dev(fallback)))
    assert (blind["views"] == 1).all() and (blind["color"][sh] == q["front"]).all() and (blind["color"][~sh] == q["back"]).all()


# ---- 4. agreement with mesh_visibility, 5. invariances

def test_the_views_bits_are_mesh_visibilitys_answers():
    case = tc.general_case()
    v, f = dev(case["vertices"]), dev(case["faces"])
    eyes = tc.eyes_of(case["RTs"])
    for form, kw in (("grid", dict(grid=F.build_mesh_grid(v, f))), ("brute", dict(vertices=v, faces=f))):
        got, ref = run(case, form=form, use_masks=False)
        seen = F.mesh_visibility(dev(case["points"]), eyes, **kw).cpu().numpy()
        reach = ~np.isin(ref["fate"], (tc.BEHIND, tc.OUTSIDE, tc.BACKFACING))
        used = (got["views"][:, None] >> np.arange(8)) & 1
        assert reach.sum() > 60 and 0 < seen[reach].sum() < reach.sum()
        assert np.array_equal(used[reach], seen[reach]), form
        assert not used[~reach].any()


def test_face_order_grid_graph_and_single_outputs_change_no_bit():
    case = tc.general_case()
    base, ref = run(case)
    brute, _ = run(case, form="brute")
    perm = np.random.default_rng(2).permutation(len(case["faces"]))
    shuffled, _ = run(dict(case, faces=np.ascontiguousarray(case["faces"][perm])))
    for other in (brute, shuffled):
        assert_same(other, base, "invariance")
    pts, img = dev(case["points"]), dev(case["images"])
    kw = dict(normals=dev(case["normals"]), masks=dev(case["masks"]), fallback=dev(case["fallback"]), z_near=case["z_near"],
              grid=F.build_mesh_grid(dev(case["vertices"]), dev(case["faces"])))
    for name in ("color", "weight", "views"):
        one = host(F.texture_points(pts, case["Ks"], case["RTs"], img, want=(name,), **kw))
        assert set(one) == {name, "stats", "totals"}
        for k in one:
            assert np.array_equal(bits(one[k]), bits(base[k])), (name, k)
    F.texture_points(pts, case["Ks"], case["RTs"], img, **kw)              # (the stream's workspace exists before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = F.texture_points(pts, case["Ks"], case["RTs"], img, **kw)
    for _ in range(2):
        for t in res.values():
            t.fill_(7)
        g.replay()
        replay = host(res)
        assert_same(replay, base, "graph replay")


# ---- 6. the pixel convention against the per-ray path

def test_the_convention_is_the_per_ray_paths(syn):
    """gpnerf_project_gather (Projector.compute: K P in float32, grid_sample align_corners=True) and texture_points name the same
    position of the same image: one view at a time, no normals, masks or mesh, C = 4 on frame.imgs.  The gather projects in float32,
    so the bound is 4 x the deviation of the restatement's float32-projection variant from its float64 form at the same points."""
    sc = syn.make_scene(H=16, W=16, seed=42, fill="full", pose="random", aabb_half=(0.12, 0.16, 0.05), bias_std=0.1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    fr = F.Frame(t(sc["src_imgs"][0]), t(sc["featmaps"]), [t(v) for v in sc["volumes"]], t(sc["src_Ks"][0]), t(sc["src_poses"][0]), sc["Rh"][0],
                 sc["Th"][0], sc["bounds"][0, 0], sc["voxel_size"], sc["out_sh"][0], F.pack_head(sc["head"], DEV))
    Ks, RTs = np.asarray(sc["src_Ks"][0], np.float64), np.asarray(sc["src_poses"][0], np.float64)[:, :3, :4]
    imgs = fr.imgs.cpu().numpy()
    V, H, W, _ = imgs.shape
    lo, hi = np.asarray(sc["bounds"][0, 0], np.float64), np.asarray(sc["bounds"][0, 1], np.float64)
    cand = (lo + np.random.default_rng(6).random((8000, 3)) * (hi - lo)).astype(np.float32)
    if sc["Rh"] is not None:                                   # the bounds are the canonical box: to the world, as the renderer does
        cand = (cand.astype(np.float64) @ np.asarray(sc["Rh"][0], np.float64).T + np.asarray(sc["Th"][0], np.float64).reshape(1, 3)).astype(np.float32)
    ref64 = tc.restate(cand, Ks, RTs, imgs, sharpness=0)
    inside = (ref64["fate"] == tc.USED).all(axis=1)
    pts = np.ascontiguousarray(cand[inside])
    assert len(pts) >= 200, f"{len(pts)} of {len(cand)} candidates are inside all {V} views"
    feat, mask = F.project_gather(fr, t(pts))
    feat, mask = feat.cpu().numpy(), mask.cpu().numpy()
    for v in range(V):
        got = host(F.texture_points(t(pts), Ks[v:v + 1], RTs[v:v + 1], fr.imgs[v:v + 1], sharpness=0))
        r64 = tc.restate(pts, Ks[v:v + 1], RTs[v:v + 1], imgs[v:v + 1], sharpness=0)
        r32 = tc.restate(pts, Ks[v:v + 1], RTs[v:v + 1], imgs[v:v + 1], sharpness=0, dtype=np.float32)
        assert_same(got, r64, ("view", v))
        assert (got["views"] == 1).all()
        agree = mask[:, v] == 1
        d32 = float(np.abs(r32["color"][:, :3].astype(np.float64) - r64["color"][:, :3]).max())
        d = float(np.abs(feat[agree, v, :3].astype(np.float64) - got["color"][agree, :3]).max())
        print(f"view {v}: {int(agree.sum())} of {len(pts)} points valid in the gather; | gather - texture | {d:.3e}; float32 variant against float64 {d32:.3e}")
        assert agree.sum() >= len(pts) - 4, "the gather's float32 frame test may differ at a point on the frame, not elsewhere"
        assert d <= 4 * d32


# ---- 7. Renderer(mesh_texture="views")

@pytest.fixture(scope="module")
def rendered():
    import os
    import sys
    from types import SimpleNamespace as NS
    from golden_cases import load, scene_of
    R = importlib.import_module("gp-nerf_amd.render")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = os.path.join(root, "gp-nerf_amd", "plugins")
    if p not in sys.path:
        sys.path.insert(0, p)
    import types
    m = types.ModuleType("fixed_encoder")

    class Enc(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("tests pass featmaps in the batch")

    m.build_encoder = lambda cfg: Enc()
    sys.modules["fixed_encoder"] = m
    hip_demo = importlib.import_module("hip_demo_render")
    _, meta = load("mesh/mesh_body")
    sc = scene_of(meta)
    cfg = NS(encoder=NS(file="fixed_encoder", name="resnet34", out_ch=32),
             head=NS(file="hip_head", rgb=NS(use_rgbhead=False),
                     sigma=NS(code_dim=32, n_heads=4, n_layers=4, n_smpl=6890, outdims=[32, 32, 32, 32])),
             dataset=NS(train=NS(name="zju_mocap", chunk=400), test=NS(name="zju_mocap", chunk=2000),
                        voxel_size=[float(x) for x in sc["voxel_size"]]),
             train=NS(n_rays=1024, n_samples=32), test=NS(mesh_th=50))
    plain = hip_demo.build_render(cfg).to(DEV).eval()
    sd = plain.state_dict()
    for k, v in sc["head"].items():
        sd["nerfhead." + k] = torch.from_numpy(v.copy())
    plain.load_state_dict(sd, strict=True)
    make = lambda mesh_th=plain.mesh_th, **kw: R.Renderer(plain.encoder, plain.nerfhead, neg_ray_train=plain.neg_ray_train,
                                                          neg_ray_val=plain.neg_ray_val, n_rays=plain.n_rays, n_samples=plain.n_samples,
                                                          voxel_size=cfg.dataset.voxel_size, mesh_th=mesh_th, progressive=True, **kw).to(DEV).eval()
    keys = ("src_imgs", "src_Ks", "src_poses", "feature", "coord", "out_sh", "bounds", "Rh", "R", "Th")
    b = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(DEV) for k in keys}
    b["featmaps"] = torch.from_numpy(sc["featmaps"]).to(DEV)
    b["volumes"] = [torch.from_numpy(v).to(DEV) for v in sc["volumes"]]
    b["target_K"] = torch.from_numpy(sc["target_K"]).to(DEV)
    b["target_pose"] = torch.from_numpy(sc["target_pose"]).to(DEV)
    with torch.no_grad():
        base = plain.render_mesh(b)
        off = make(mesh_texture=0).render_mesh(b)
        coloured = make(mesh_colors=True).render_mesh(b)
        textured = make(mesh_texture="views").render_mesh(b)
        # the dense renderer's geometry mode on the same frame: the dataset's lattice over can_bounds, every point kept
        axes = F.dataset_lattice_axes(sc["can_bounds"][0], sc["voxel_size"])
        pts = torch.from_numpy(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).astype(np.float32)).to(DEV)
        g = dict(b, pts=pts[None], inside=torch.ones(pts.shape[:3], dtype=torch.uint8, device=DEV)[None])
        geo_coloured = make(mesh_th=1.0 / 50.0, mesh_colors=True).render_geometry(g)
        geo_textured = make(mesh_th=1.0 / 50.0, mesh_texture="views").render_geometry(g)
    return NS(base=base, off=off, coloured=coloured, textured=textured, geo_coloured=geo_coloured, geo_textured=geo_textured)


def test_render_mesh_with_the_option_off_is_todays(rendered):
    base, off = rendered.base, rendered.off
    assert set(base) == set(off) and "mesh_stats" not in off
    assert np.array_equal(base["cube"].view(np.uint32), off["cube"].view(np.uint32))
    assert np.array_equal(base["mesh"].vertices, off["mesh"].vertices) and np.array_equal(base["mesh"].faces, off["mesh"].faces)
    assert off["mesh"].vertex_colors is None and off["mesh"].vertex_normals is None


@pytest.mark.parametrize("mode", ["render_mesh", "render_geometry"])
def test_the_renderer_takes_its_colours_from_the_views(rendered, mode):
    tex, col = (rendered.textured, rendered.coloured) if mode == "render_mesh" else (rendered.geo_textured, rendered.geo_coloured)
    m, s = tex["mesh"], tex["mesh_stats"]
    nv = len(m.vertices)
    assert np.array_equal(m.vertices, col["mesh"].vertices) and np.array_equal(m.faces, col["mesh"].faces) and m.vertex_normals is None
    c = m.vertex_colors
    assert c.shape == (nv, 3) and c.dtype == np.float32 and np.isfinite(c).all() and c.min() >= 0.0 and c.max() <= 1.0
    for name in L.TEXTURE_STATS:
        assert len(s[f"texture_{name}"]) == 3
    rows = np.array([s[f"texture_{name}"] for name in L.TEXTURE_STATS])
    assert (rows.sum(axis=0) == nv).all() and s["texture_seen"] + s["texture_unseen"] == nv
    changed = (c.view(np.uint32) != col["mesh"].vertex_colors.view(np.uint32)).any(axis=1)
    print(f"{mode}(mesh_texture='views'): {nv} vertices, seen {s['texture_seen']}, unseen {s['texture_unseen']}, "
          f"{int(changed.sum())} colours differ from the field's;", {k: v for k, v in s.items() if k.startswith("texture_")})
    assert s["texture_seen"] > 0 and changed.sum() <= s["texture_seen"]
    assert (~changed).sum() >= s["texture_unseen"], "a vertex no view sees keeps the field's colour bit for bit"


# ---- 8. MeshEvaluator(texture=True)

def _texture_frame(swap=False, size=40):
    import raster_cases as ras
    import raycast_cases as rc
    import voxelize_cases as vc
    ev = importlib.import_module("gp-nerf_amd.evaluator")
    M = importlib.import_module("gp-nerf_amd.mesh")
    pad = ev.MeshEvaluator.PAD
    axes = [np.linspace(-0.6, 0.6, 13).astype(np.float32), np.linspace(-0.5, 0.7, 13).astype(np.float32), np.linspace(-0.6, 0.6, 13).astype(np.float32)]
    centre = np.array([pad + 6.2, pad + 5.7, pad + 6.4])
    pred = M.Mesh(*vc.placed_sphere(2, 4.0, centre))
    world = pred.to_lattice_frame(axes, pad)
    mid = world.vertices.mean(axis=0)
    colours = (0.5 + 0.4 * (world.vertices - mid) / np.abs(world.vertices - mid).max()).astype(np.float32)
    cams = [rc.look_at(mid + 2.0 * np.array([np.cos(a), np.sin(a), 0.35 * (-1) ** k]), mid, size, size, 1.6 * size)
            for k, a in enumerate(2 * np.pi * np.arange(8) / 8 + 0.2)]
    Ks, RTs = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    v, f = F.mesh_to_device(world, torch.device(DEV))
    drawn = F.rasterize_mesh(v, f, Ks, RTs, size, size, want=("face_id",), attributes=dev(colours))
    imgs, masks = drawn["image"], (drawn["face_id"] >= 0).to(torch.uint8)
    if swap:
        imgs = imgs.clone()
        imgs[[0, 4]] = imgs[[0, 4]][..., [2, 0, 1]]
    batch = {"frame_index": torch.tensor([0]), "hull_masks": masks[None], "hull_imgs": imgs[None].contiguous(),
             "hull_Ks": torch.from_numpy(Ks)[None], "hull_RTs": torch.from_numpy(RTs)[None]}
    return {"cube": np.pad(np.zeros((13, 13, 13), np.float32), pad), "mesh": pred, "axes": axes}, batch, (world, Ks, RTs, ras)


def test_mesh_evaluator_texture_end_to_end(tmp_path):
    ev = importlib.import_module("gp-nerf_amd.evaluator")
    got = {}
    for swap in (False, True):
        output, batch, (world, Ks, RTs, ras) = _texture_frame(swap)
        e = ev.MeshEvaluator(str(tmp_path / str(swap)), 0.02, texture=True, texture_holdout=4)
        e.evaluate(output, batch)
        assert e.has_mesh_metrics
        got[swap] = e.summarize()
        assert not e.has_mesh_metrics
    res = got[False]
    table = np.load(tmp_path / "False" / "texture_metrics.npy")
    assert table["frame_index"].tolist() == [0] and table["pixels"][0] == res["texture_pixels"] > 200
    assert np.isfinite(res["texture_psnr"]) and res["per_frame"]["texture_frame_index"] == [0] and 0 < res["texture_seen_fraction"] <= 1
    assert got[True]["texture_psnr"] < res["texture_psnr"] - 3.0, (got[True]["texture_psnr"], res["texture_psnr"])
    # the same pipeline restated in float64 on the host: colours (texture_cases.restate with the faces' area-weighted normals), the
    # rasteriser and its interpolation (raster_cases), the masked mean square
    output, batch, _ = _texture_frame(False)
    imgs, masks = batch["hull_imgs"][0].cpu().numpy(), batch["hull_masks"][0].cpu().numpy()
    wv, wf = world.vertices.astype(np.float32), world.faces
    source, held = [1, 2, 3, 5, 6, 7], [0, 4]
    v64 = wv.astype(np.float64)
    fn = np.cross(v64[wf[:, 1]] - v64[wf[:, 0]], v64[wf[:, 2]] - v64[wf[:, 0]])
    nrm = np.zeros_like(v64)
    for k in range(3):
        np.add.at(nrm, wf[:, k], fn)
    ref = tc.restate(wv, Ks[source], RTs[source], imgs[source], normals=nrm.astype(np.float32), masks=masks[source], vertices=wv, faces=wf)
    cams = np.concatenate([Ks[held].reshape(-1, 9), RTs[held].reshape(-1, 12)], axis=1)
    size = imgs.shape[1]
    fid = ras.rasterize_np(wv, wf, cams, size, size, z_near=1e-6)["face_id"]
    image = ras.interpolate_np(fid, wv, wf, cams, size, size, ref["color"], 0.0, z_near=1e-6)
    counted = (fid >= 0) & (masks[held] == 1)
    diff = (image.astype(np.float32) - imgs[held])[counted].astype(np.float64)
    want = -10.0 * np.log10((diff * diff).mean())
    print(f"texture_psnr {res['texture_psnr']:.6f} dB over {res['texture_pixels']} pixels, float64 restatement {want:.6f} dB; "
          f"channels swapped {got[True]['texture_psnr']:.3f} dB; seen fraction {res['texture_seen_fraction']:.4f}")
    assert int(counted.sum()) == res["texture_pixels"]
    assert abs(res["texture_psnr"] - want) <= 1e-5 * abs(want)


def test_texture_off_changes_nothing_and_missing_keys_raise(tmp_path):
    ev = importlib.import_module("gp-nerf_amd.evaluator")
    output, batch, _ = _texture_frame()
    plain = ev.MeshEvaluator(str(tmp_path / "plain"), 0.02)
    plain.evaluate(output, batch)
    assert not plain.has_mesh_metrics and plain.summarize() == {}
    on = ev.MeshEvaluator(str(tmp_path / "on"), 0.02, texture=True)
    for key in ev.MeshEvaluator.TEXTURE_KEYS:
        with pytest.raises(L.GpnerfError, match=rf"texture=True.*'{key}'"):
            on.evaluate(output, {k: v for k, v in batch.items() if k != key})
    with pytest.raises(L.GpnerfError, match="axes"):
        on.evaluate({"cube": output["cube"], "mesh": output["mesh"]}, dict(batch, pts=torch.zeros((1, 13, 13, 13, 3))))
    with pytest.raises(L.GpnerfError, match="texture_holdout"):
        ev.MeshEvaluator(str(tmp_path / "bad"), 0.02, texture=True, texture_holdout=1)
