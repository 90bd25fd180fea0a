"""GPU: the dense renderer's geometry mode (BaseRender.py:255-272, use_rgbhead False) -- the visual-hull kernel against the
reference's own prepare_inside_pts runs (tests/golden/hull/) and the numpy restatement (tests/hull_cases.py), the masked density
lattice against gpnerf_query_points bit for bit, `render.file hip_render` with both batch routes, and the evaluation loop with a
MeshEvaluator."""
import ctypes as C
import importlib
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import hull_cases as hc
from golden_cases import load, scene_of, sha_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = importlib.import_module("gp-nerf_amd.frame")
L = importlib.import_module("gp-nerf_amd._lib")
ev = importlib.import_module("gp-nerf_amd.evaluator")
DEV = "cuda:0"
PAD = F.MESH_PAD


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the hull kernel ---------------------------------------------------------------------------------------------------------------
def hull_raw(axes, masks, cams, out, n_inside, n_views=None):
    """gpnerf_visual_hull into caller-made buffers; returns the entry point's code"""
    ax = [t(np.asarray(a, np.float32)) for a in axes]
    m = t(masks)
    cams = np.ascontiguousarray(cams, dtype=np.float64)
    dims = (C.c_int32 * 3)(*[len(a) for a in axes])
    code = L.lib().gpnerf_visual_hull(ax[0].data_ptr(), ax[1].data_ptr(), ax[2].data_ptr(), dims, masks.shape[0] if n_views is None else n_views,
                                      m.data_ptr(), masks.shape[1], masks.shape[2], cams.ctypes.data_as(L.DP), out.data_ptr(),
                                      n_inside.data_ptr() if n_inside is not None else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize("name", hc.hull_case_names())
def test_hull_kernel_is_the_reference_fixture(name):
    z, meta, axes = hc.load_hull(name)
    _, tie, _ = hc.hull_np(axes, z["masks"], z["cams"])
    inside, n_inside = F.visual_hull(axes, t(z["masks"]), z["cams"][:, :9], z["cams"][:, 9:])
    got = inside.cpu().numpy()
    left_out = hc.compare_outside_ties(got, z["inside"], tie)
    assert int(n_inside.item()) == int(np.count_nonzero(got))
    print(f"{name}: {got.size} points, {left_out} left out, n_inside {int(n_inside.item())}, values {dict(zip(*np.unique(got, return_counts=True)))}")


@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 7, 13), (3, 5, 130), (2, 3, 4)])
@pytest.mark.parametrize("offset", [0, 1])
def test_hull_kernel_is_the_restatement_on_small_lattices(dims, offset):
    """Z tail, Z < 4, rows whose base is not 4-aligned (and, offset 1, an output that is not 4-aligned itself: byte stores); every
    element written (a prefilled output), nothing written past the end"""
    z, meta, axes = hc.load_hull("hull_body")
    sub = [axes[0][20:20 + dims[0]], axes[1][30:30 + dims[1]], np.linspace(axes[2][0], axes[2][-1], dims[2]).astype(np.float32)]
    ref, tie, _ = hc.hull_np(sub, z["masks"], z["cams"])
    assert not tie.any() and ref.shape == dims
    n = int(np.prod(dims))
    buf = torch.full((n + 16,), 0xCD, device=DEV, dtype=torch.uint8)
    out = buf[offset:offset + n]
    n_inside = torch.full((1,), -7, device=DEV, dtype=torch.int64)
    assert hull_raw(sub, z["masks"], z["cams"], out, n_inside) == 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[offset:offset + n].reshape(dims), ref)
    assert (got[:offset] == 0xCD).all() and (got[offset + n:] == 0xCD).all()
    assert int(n_inside.item()) == int(np.count_nonzero(ref))


def test_hull_kernel_refuses_bad_arguments():
    z, meta, axes = hc.load_hull("hull_one")
    out = torch.zeros(tuple(len(a) for a in axes), device=DEV, dtype=torch.uint8)
    masks9 = np.repeat(z["masks"], 9, axis=0)
    cams9 = np.repeat(z["cams"], 9, axis=0)
    assert hull_raw(axes, masks9, cams9, out, None, n_views=0) == -1
    assert hull_raw(axes, masks9, cams9, out, None, n_views=9) == -1
    assert hull_raw(axes, masks9, cams9, out, None, n_views=8) == 0
    with pytest.raises(L.GpnerfError):
        F.visual_hull(axes, t(masks9), cams9[:, :9], cams9[:, 9:])
    with pytest.raises(L.GpnerfError):
        F.visual_hull(axes, t(z["masks"]), cams9[:, :9], cams9[:, 9:])          # 1 mask, 9 cameras


# ---- the masked lattice ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def body():
    """the mesh_body synthetic frame (tests/golden/mesh/mesh_body.npz's scene) WITHOUT an occupancy volume, and a 5 mm hull lattice
    (dataset_lattice_axes) over the box the reference found for it"""
    z, meta = load("mesh/mesh_body")
    sc = scene_of(meta)
    assert sha_inputs(sc) == meta["sha256_inputs"]
    blob = F.pack_head(sc["head"], torch.device(DEV))
    fr = F.Frame(t(sc["src_imgs"][0]), t(sc["featmaps"]), [t(v) for v in sc["volumes"]], t(sc["src_Ks"][0]), t(sc["src_poses"][0]),
                 sc["Rh"][0], sc["Th"][0], sc["bounds"][0, 0], sc["voxel_size"], sc["out_sh"][0], blob)
    box = np.asarray(z["can_bounds"], np.float32)
    axes = F.dataset_lattice_axes(box, [float(v) for v in sc["voxel_size"]])
    return NS(sc=sc, fr=fr, box=box, axes=axes, meta=meta, alpha={})


def reference_cube(b, axes, inside):
    """query_points (density only, alpha, no cull) at the kept points, scattered into a zero padded cube"""
    sh = tuple(len(a) for a in axes)
    key = (sh, tuple(float(a[0]) for a in axes), tuple(float(a[-1]) for a in axes))
    if key not in b.alpha:                                   # the whole lattice once; a point's result depends on that point alone
        pts = t(hc.lattice_points(axes))
        b.alpha[key] = F.query_points(b.fr, pts, want=("sigma", "alpha"))["alpha"].cpu().numpy().reshape(sh)
    cube = np.zeros(tuple(s + 2 * PAD for s in sh), np.float32)
    cube[PAD:-PAD, PAD:-PAD, PAD:-PAD] = np.where(inside != 0, b.alpha[key], np.float32(0))
    return cube


def masked_raw(fr, axes, inside, pad=PAD):
    """gpnerf_density_lattice_masked into a NaN-prefilled cube"""
    sh = tuple(len(a) for a in axes)
    ax = [t(np.asarray(a, np.float32)) for a in axes]
    cube = torch.full(tuple(s + 2 * pad for s in sh), float("nan"), device=DEV)
    n_kept = torch.full((1,), -3, device=DEV, dtype=torch.int64)
    ins = t(np.asarray(inside, np.uint8))
    dims = (C.c_int32 * 3)(*sh)
    L.check(L.lib().gpnerf_density_lattice_masked(C.byref(fr.c), ax[0].data_ptr(), ax[1].data_ptr(), ax[2].data_ptr(), dims, pad, 0,
                                                  ins.data_ptr(), cube.data_ptr(), n_kept.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "gpnerf_density_lattice_masked")
    torch.cuda.synchronize()
    return cube.cpu().numpy(), int(n_kept.item())


def one_lane_per_brick(sh):
    """exactly one point of every 4 (y) x 8 (z) brick of the padded cube's x-slices, where that lane lies inside the lattice"""
    i, j, k = np.meshgrid(*[np.arange(s) for s in sh], indexing="ij")
    y, z = j + PAD, k + PAD
    lane = (y % 4) * 8 + z % 8
    chosen = ((i + PAD) * 7 + (y // 4) * 13 + (z // 8) * 5) % 32
    return (lane == chosen).astype(np.uint8)


def body_carve(axes, box):
    """the hull_body masks and cameras, re-centred on this lattice's box"""
    z, meta, haxes = hc.load_hull("hull_body")
    shift = 0.5 * (box[0] + box[1]).astype(np.float64) - np.array([0.5 * (np.float64(a[0]) + np.float64(a[-1])) for a in haxes])
    cams = z["cams"].copy()
    for c in cams:
        RT = c[9:].reshape(3, 4)
        RT[:, 3] -= RT[:, :3] @ shift
    return z["masks"], cams


MASKS = ["ones", "zeros", "one_point", "checkerboard", "one_lane_per_brick", "values_100_255", "hull_body"]


@pytest.mark.parametrize("kind", MASKS)
def test_masked_lattice_is_query_points_bit_for_bit(body, kind):
    axes, sh = body.axes, tuple(len(a) for a in body.axes)
    i, j, k = np.meshgrid(*[np.arange(s) for s in sh], indexing="ij")
    if kind == "ones":
        inside = np.ones(sh, np.uint8)
    elif kind == "zeros":
        inside = np.zeros(sh, np.uint8)
    elif kind == "one_point":
        inside = np.zeros(sh, np.uint8)
        inside[sh[0] // 2, sh[1] // 2 + 1, sh[2] // 2] = 1
    elif kind == "checkerboard":
        inside = ((i + j + k) % 2).astype(np.uint8)
    elif kind == "one_lane_per_brick":
        inside = one_lane_per_brick(sh)
    elif kind == "values_100_255":
        inside = np.choose((i * 5 + j * 3 + k) % 4, [0, 100, 255, 0]).astype(np.uint8)
    else:
        masks, cams = body_carve(axes, body.box)
        ins_dev, n_dev = F.visual_hull(axes, t(masks), cams[:, :9], cams[:, 9:])
        ref, tie, _ = hc.hull_np(axes, masks, cams)
        inside = ins_dev.cpu().numpy()
        hc.compare_outside_ties(inside, ref, tie)
        assert set(np.unique(inside)) == {0, 1, 100}
    assert not body.fr.c.occ, "the masked lattice needs no occupancy volume"
    want = reference_cube(body, axes, inside)
    got, n_kept = masked_raw(body.fr, axes, inside)
    assert not np.isnan(got).any(), "every element of the cube is written"
    assert n_kept == int(np.count_nonzero(inside))
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), int((got.view(np.int32) != want.view(np.int32)).sum())
    if kind == "zeros":
        assert not got.any() and n_kept == 0
    if kind == "ones":
        assert (got > 0.02).any() and (got[PAD:-PAD, PAD:-PAD, PAD:-PAD] < 0.02).any(), "the frame has a surface"
    # the wrapper takes the same entry point, and two runs give the same bits
    cube2, n2 = F.density_lattice(body.fr, axes, inside=t(inside))
    assert np.array_equal(cube2.cpu().numpy().view(np.int32), got.view(np.int32)) and int(n2.item()) == n_kept
    assert not body.fr.c.occ
    print(f"{kind}: lattice {sh}, kept {n_kept}")


@pytest.mark.parametrize("dims", [(5, 7, 13), (3, 5, 130)])
def test_masked_lattice_bricks_that_straddle_the_padding(body, dims):
    lo, hi = body.box[0].astype(np.float64), body.box[1].astype(np.float64)
    axes = [np.linspace(lo[a] + 0.2 * (hi[a] - lo[a]), hi[a] - 0.2 * (hi[a] - lo[a]), dims[a]).astype(np.float32) for a in range(3)]
    i, j, k = np.meshgrid(*[np.arange(s) for s in dims], indexing="ij")
    for inside in (np.ones(dims, np.uint8), ((i + 2 * j + k) % 3 != 0).astype(np.uint8)):
        want = reference_cube(body, axes, inside)
        got, n_kept = masked_raw(body.fr, axes, inside)
        assert not np.isnan(got).any() and n_kept == int(np.count_nonzero(inside))
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert want.any()


def test_masked_lattice_refuses_bad_arguments(body):
    sh = tuple(len(a) for a in body.axes)
    with pytest.raises(L.GpnerfError):
        F.density_lattice(body.fr, body.axes, inside=torch.ones((sh[0], sh[1], sh[2] + 1), device=DEV, dtype=torch.uint8))
    with pytest.raises(L.GpnerfError):
        F.density_lattice(body.fr, body.axes, inside=torch.ones(sh, device=DEV, dtype=torch.float32))


# ---- `render.file hip_render`, use_rgbhead False --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def renderer(body):
    p = os.path.join(ROOT, "gp-nerf_amd", "plugins")
    if p not in sys.path:
        sys.path.insert(0, p)
    import types
    m = types.ModuleType("fixed_encoder")

    class Enc(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("tests pass featmaps in the batch")

    m.build_encoder = lambda cfg: Enc()
    sys.modules["fixed_encoder"] = m
    hip_render = importlib.import_module("hip_render")
    sc = body.sc
    cfg = NS(encoder=NS(file="fixed_encoder", name="resnet34", out_ch=32),
             head=NS(file="hip_head", rgb=NS(use_rgbhead=False),
                     sigma=NS(code_dim=32, n_heads=4, n_layers=4, n_smpl=6890, outdims=[32, 32, 32, 32])),
             dataset=NS(train=NS(name="zju_mocap", chunk=400), test=NS(name="zju_mocap", chunk=2000),
                        voxel_size=[float(x) for x in sc["voxel_size"]]),
             train=NS(n_rays=1024, n_samples=32), test=NS(mesh_th=50, test_seq="s"))
    r = hip_render.build_render(cfg).to(DEV).eval()
    assert r.nerfhead.use_rgbhead is False and r.mesh_th == 1 / 50
    sd = r.state_dict()
    for k, v in sc["head"].items():
        sd["nerfhead." + k] = torch.from_numpy(v.copy())
    r.load_state_dict(sd, strict=True)
    keys = ("src_imgs", "src_Ks", "src_poses", "feature", "coord", "out_sh", "bounds", "Rh", "R", "Th")
    base = {k: t(sc[k]) for k in keys}
    base["featmaps"] = t(sc["featmaps"])
    base["volumes"] = [t(v) for v in sc["volumes"]]
    masks, cams = body_carve(body.axes, body.box)
    ref, tie, _ = hc.hull_np(body.axes, masks, cams)
    assert not tie.any(), "a case with no left-out point"
    route_a = dict(base, pts=t(hc.lattice_points(body.axes).reshape(tuple(len(a) for a in body.axes) + (3,)))[None], inside=t(ref)[None])
    route_b = dict(base, hull_masks=t(masks)[None], hull_Ks=t(cams[:, :9].reshape(-1, 3, 3))[None],
                   hull_RTs=t(cams[:, 9:].reshape(-1, 3, 4))[None], can_bounds=t(body.box)[None])
    with torch.no_grad():
        ret_a = r.render(route_a)
    return NS(r=r, cfg=cfg, base=base, route_a=route_a, route_b=route_b, inside=ref, ret_a=ret_a)


def test_renderer_route_a_is_the_masked_lattice_and_its_mesh(body, renderer):
    ret = renderer.ret_a
    assert {"cube", "mesh", "axes", "n_inside", "time_slots", "etime", "rtime"} <= set(ret) and "rgb_map" not in ret and "mesh_stats" not in ret
    cube = ret["cube"]
    assert isinstance(cube, np.ndarray) and cube.dtype == np.float32
    for a, b in zip(ret["axes"], body.axes):
        assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    want, n_kept = F.density_lattice(body.fr, body.axes, inside=t(renderer.inside), pad=10)
    assert np.array_equal(cube.view(np.int32), want.cpu().numpy().view(np.int32))
    assert ret["n_inside"] == int(n_kept.item()) == int(np.count_nonzero(renderer.inside))
    v, f = F.marching_cubes(want, 1 / renderer.cfg.test.mesh_th)
    m = ret["mesh"]
    assert len(m.faces) > 100
    assert np.array_equal(m.vertices, v.cpu().numpy().astype(np.float64)) and np.array_equal(m.faces, f.cpu().numpy().astype(np.int64))
    assert ret["rtime"] > 0 and ret["etime"] >= 0


def test_renderer_route_b_carves_on_the_device_and_equals_route_a(renderer):
    with torch.no_grad():
        ret = renderer.r.render(renderer.route_b)
    a = renderer.ret_a
    assert np.array_equal(ret["cube"].view(np.int32), a["cube"].view(np.int32)) and ret["n_inside"] == a["n_inside"]
    assert np.array_equal(ret["mesh"].vertices, a["mesh"].vertices) and np.array_equal(ret["mesh"].faces, a["mesh"].faces)
    for x, y in zip(ret["axes"], a["axes"]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_renderer_names_the_missing_keys(renderer):
    for drop in ({"inside"}, {"pts"}):
        b = {k: v for k, v in renderer.route_a.items() if k not in drop}
        with pytest.raises(L.GpnerfError, match="hull_masks"):
            renderer.r.render(b)
    b = {k: v for k, v in renderer.route_b.items() if k != "hull_RTs"}
    with pytest.raises(L.GpnerfError, match="'pts' and 'inside'"):
        renderer.r.render(b)


def test_renderer_mesh_clean_largest_is_a_subset(renderer):
    r = renderer.r
    saved = r.mesh_clean
    r.mesh_clean = "largest"
    try:
        with torch.no_grad():
            ret = r.render(renderer.route_a)
    finally:
        r.mesh_clean = saved
    plain = renderer.ret_a["mesh"]
    tri = lambda m: {m.vertices[f].tobytes() for f in m.faces}
    sub, full = tri(ret["mesh"]), tri(plain)
    assert 0 < len(sub) <= len(full) and sub <= full
    assert "mesh_stats" in ret and ret["mesh_stats"]["components_kept"] == 1 and ret["mesh_stats"]["components"] >= 1
    assert np.array_equal(ret["cube"].view(np.int32), renderer.ret_a["cube"].view(np.int32)), "`cube` stays the untouched one"


def test_evaluate_loop_with_a_mesh_evaluator(renderer, tmp_path):
    loader = [dict(renderer.route_a, frame_index=torch.tensor([3])), dict(renderer.route_b, frame_index=torch.tensor([4]))]
    e = ev.MeshEvaluator(str(tmp_path), renderer.r.mesh_th, export_mesh=True)
    res = ev.evaluate_loop(renderer.r, loader, renderer.cfg, quiet=True, evaluator=e)
    assert res["count"] == 2 and res["metrics"] is None and res["mse"] == [] and res["total_time"] > 0
    assert sorted(os.listdir(tmp_path / "pts")) == ["3.npy", "4.npy"] and sorted(os.listdir(tmp_path / "mesh")) == ["3.ply", "4.ply"]
    a, b = np.load(tmp_path / "pts" / "3.npy"), np.load(tmp_path / "pts" / "4.npy")
    inner = renderer.ret_a["cube"][10:-10, 10:-10, 10:-10]
    assert a.dtype == np.float32 and len(a) == int((inner > renderer.r.mesh_th).sum()) > 0
    assert np.array_equal(a, b), "the points from batch['pts'] and from the output's axes are the same"
