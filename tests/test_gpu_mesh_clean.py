"""GPU: finishing the extracted mesh on the device -- gpnerf_cube_clean (solid components, floaters, cavities) exactly equal to the
numpy / scipy restatement (tests/mesh_clean_cases.py) on cubes chosen for the union-find's hard cases, determinism and graph capture,
gpnerf_mesh_normals against the float64 restatement, and Renderer.render_mesh end to end."""
import ctypes as C
import functools
import importlib
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import mesh_cases as mc
import mesh_clean_cases as cc
from golden_cases import load, scene_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
R = importlib.import_module("gp-nerf_amd.render")
L = importlib.import_module("gp-nerf_amd._lib")
DEV = "cuda:0"
ISO = M.ISO_REFERENCE
GOLDEN = ["mesh/mesh_body", "mesh/mesh_trained"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(cube float32, iso) of a named case; built once"""
    if name in GOLDEN:
        return np.ascontiguousarray(load(name)[0]["cube"], dtype=np.float32), ISO
    small = cc.small_cubes()
    table = {
        "noise": lambda: (cc.noise_cube(), 0.02),                          # the solid percolates; hundreds of cavities
        "noise_ties": lambda: (cc.noise_cube(), cc.NOISE_TIE_ISO),         # thousands of components; the tie rule decides "largest"
        "snakes": lambda: (cc.snakes_cube(), 0.5),                         # the longest union chains; a tie between the two
        "diagonals": lambda: (cc.diagonal_pairs_cube()[0], 0.5),           # face diagonals join, body diagonals do not, across bricks
        "d222": lambda: (small["d222"], 0.02),
        "d35130": lambda: (small["d35130"], 0.02),
        "all_inside": lambda: (small["all_inside"], 0.5),
        "all_outside": lambda: (small["all_outside"], 0.5),
        "faces": lambda: (cc.faces_touching_cube(), 0.5),
        "shell": lambda: (cc.shell_cube(), 0.5),                           # filled
        "shell_tunnel": lambda: (cc.shell_cube(tunnel=True), 0.5),         # not filled
        "shell_diagonal": lambda: (cc.shell_cube(diagonal_leak=True), 0.5),  # filled: 6-connectivity does not leak across a diagonal
        "floater_bubble": lambda: (cc.floater_bubble_cube(), 0.5),         # KEEP removes the floater, its bubble has opened
    }
    return table[name]()


CASES = GOLDEN + ["noise", "noise_ties", "snakes", "diagonals", "d222", "d35130", "all_inside", "all_outside", "faces", "shell",
                  "shell_tunnel", "shell_diagonal", "floater_bubble"]


@functools.lru_cache(maxsize=None)
def restated(name, mode):
    cube, iso = case(name)
    flags, min_points = cc.MODES[mode]
    return cc.clean_np(cube, iso, flags, min_points)


def device_clean(cube, iso, mode, want_labels=True):
    flags, min_points = cc.MODES[mode]
    keep = None if not flags & cc.KEEP else (min_points or "largest")
    out, stats, labels = F.cube_clean(torch.from_numpy(cube).to(DEV), iso, keep=keep, fill_cavities=bool(flags & cc.FILL), want_labels=want_labels)
    return out.cpu().numpy(), stats.cpu().numpy(), labels.cpu().numpy() if labels is not None else None


@pytest.mark.parametrize("mode", sorted(cc.MODES))
@pytest.mark.parametrize("name", CASES)
def test_cube_clean_is_the_restatement_exactly(name, mode):
    cube, iso = case(name)
    ref_out, ref_labels, ref_stats = restated(name, mode)
    out, stats, labels = device_clean(cube, iso, mode)
    print(f"{name} {cube.shape} {mode}: stats {dict(zip(cc.STATS, stats.tolist()))}")
    assert np.array_equal(stats, ref_stats), (stats, ref_stats)
    assert np.array_equal(labels, ref_labels), f"{int((labels != ref_labels).sum())} labels differ"
    assert np.array_equal(out.view(np.uint32), ref_out.view(np.uint32)), f"{int((out.view(np.uint32) != ref_out.view(np.uint32)).sum())} values differ"


def test_the_cases_exercise_what_they_are_for():
    """the restatement's own counts on the small cases (the device equals them above): ties, diagonals, cavities, the opened bubble"""
    assert restated("snakes", "largest")[2][0] == 2 and restated("snakes", "largest")[1].max() > 0
    s_out, s_lab, s_st = restated("snakes", "largest")
    assert s_st[3] * 2 == s_st[1] and s_out[0, 0, 1] == 1 and s_out[2, 2, 1] == 0, "equal lengths: the lower label stays"
    assert restated("diagonals", "fill")[2][0] == 16
    assert restated("noise_ties", "largest")[2][0] > 2000
    assert restated("shell", "fill")[2][4] == 1 and restated("shell_tunnel", "fill")[2][4] == 0 and restated("shell_diagonal", "fill")[2][4] == 2
    assert restated("floater_bubble", "fill")[2][4] == 1 and restated("floater_bubble", "both")[2][4] == 0
    assert list(restated("all_outside", "both")[2]) == [0] * 6 and list(restated("all_inside", "both")[2][:4]) == [1, 5 * 9 * 33, 1, 5 * 9 * 33]
    assert restated("faces", "fill")[2][4] == 0 and restated("faces", "largest")[2][0] == 4


def test_no_flags_keeps_everything_and_labels_are_optional():
    cube, iso = case("noise_ties")
    ref_out, ref_labels, ref_stats = cc.clean_np(cube, iso, 0, 0)
    out, stats, labels = F.cube_clean(torch.from_numpy(cube).to(DEV), iso)
    assert labels is None and np.array_equal(stats.cpu().numpy(), ref_stats) and ref_stats[2] == ref_stats[0]
    assert np.array_equal(out.cpu().numpy().view(np.uint32), cube.view(np.uint32))


@pytest.mark.parametrize("name", GOLDEN + ["noise"])
def test_the_cleaned_mesh_is_a_subset_of_the_unfiltered_mesh(name):
    cube, iso = case(name)
    d = torch.from_numpy(cube).to(DEV)
    v, f = F.marching_cubes(d, iso)
    out, _, _ = F.cube_clean(d, iso, keep="largest", fill_cavities=True)
    cv, cf = F.marching_cubes(out, iso)
    v, f, cv, cf = v.cpu().numpy(), f.cpu().numpy().astype(np.int64), cv.cpu().numpy(), cf.cpu().numpy().astype(np.int64)
    assert 0 < len(cf) < len(f)
    assert cc.is_subset(cc.triangle_set(cv, cf), cc.triangle_set(v, f)), "positions must be the unfiltered mesh's, bit for bit"
    n = cc.surfaces(cf, len(cv))
    print(f"{name}: {cc.surfaces(f, len(v))} surfaces, {len(f)} triangles -> {n} surface(s), {len(cf)} triangles")
    if name in GOLDEN:
        assert n == 1


def _raw_call(lib, cube, dims, iso, flags, min_points, ws, out, labels, stats):
    return lib.gpnerf_cube_clean(cube.data_ptr(), dims, float(iso), flags, min_points, ws.data_ptr(), ws.numel(), out.data_ptr(),
                                 labels.data_ptr(), stats.data_ptr(), torch.cuda.current_stream().cuda_stream)


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    lib = L.lib()
    cube_np, iso = case("mesh/mesh_trained")
    cube = torch.from_numpy(cube_np).to(DEV)
    verts, _ = F.marching_cubes(cube, iso)
    dims = (C.c_int32 * 3)(*cube.shape)
    ws = torch.empty((int(lib.gpnerf_cube_clean_workspace_bytes(dims)),), device=DEV, dtype=torch.uint8)
    out, labels = torch.empty_like(cube), torch.empty(tuple(cube.shape), device=DEV, dtype=torch.int32)
    stats = torch.empty((6,), device=DEV, dtype=torch.int64)
    normals = torch.empty_like(verts)
    flags = L.CUBE_KEEP | L.CUBE_FILL
    runs = []
    for fill in (0x00, 0xFF):                               # the workspace carries nothing from call to call
        ws.fill_(fill)
        assert _raw_call(lib, cube, dims, iso, flags, 0, ws, out, labels, stats) == 0
        runs.append((out.clone(), labels.clone(), stats.clone(), F.mesh_normals(cube, verts)))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = _raw_call(lib, cube, dims, iso, flags, 0, ws, out, labels, stats)
        rn = lib.gpnerf_mesh_normals(cube.data_ptr(), dims, verts.data_ptr(), verts.shape[0], None, normals.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and rn == 0
    for _ in range(2):
        ws.fill_(0xA5)
        out.fill_(-1.0); labels.fill_(-7); stats.fill_(-1); normals.fill_(9.0)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip((out, labels, stats, normals), runs[0]):
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                               want.view(torch.int32) if want.dtype == torch.float32 else want)


# ---- normals -------------------------------------------------------------------------------------------------------------------------
def _normals_check(field, verts, inv_step=None, label=""):
    """The device within 4 x d32 of the float64 restatement, d32 = the float32 numpy restatement's own distance from it (the factor
    allows for the other rounding of the reciprocal square root); vertices whose float64 |g| is below 1e-3 max|f| -- at most 1 % --
    are checked for finiteness only."""
    n64, len64 = cc.normals_np(field, verts, inv_step, np.float64)
    n32, _ = cc.normals_np(field, verts, inv_step, np.float32)
    step = None if inv_step is None else [1.0 / float(s) for s in inv_step]
    got = F.mesh_normals(torch.from_numpy(field).to(DEV), torch.from_numpy(verts).to(DEV), step=step).cpu().numpy()
    weak = len64 < 1e-3 * float(np.abs(field).max())
    assert weak.mean() <= 0.01, f"{weak.mean():.4f} of the vertices have no usable gradient in the restatement itself"
    assert np.all(np.isfinite(got))
    d32 = float(np.abs(n32.astype(np.float64) - n64)[~weak].max())
    dev = float(np.abs(got.astype(np.float64) - n64)[~weak].max())
    same = float(np.mean(got.view(np.uint32) == n32.view(np.uint32)))
    print(f"normals {label}: {len(verts)} points, {int(weak.sum())} weak, d32 {d32:.3e}, device {dev:.3e} (bound {4 * d32:.3e}), "
          f"{same:.4f} of the words equal the float32 restatement's")
    assert d32 > 0 and dev <= 4 * d32
    assert np.all(np.abs(np.linalg.norm(got[~weak].astype(np.float64), axis=1) - 1) < 1e-6)
    return got, weak


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_normals_are_the_float64_restatement_within_float32_rounding(name):
    field = mc.sphere_field() if name == "sphere" else mc.torus_field()
    verts, _ = mc.marching_cubes_np(field, 0.02)
    got, weak = _normals_check(field, verts, label=name)
    if name == "sphere":
        n = field.shape[0]
        centre = np.array([(n - 1) / 2 + 0.31, (n - 1) / 2 - 0.17, (n - 1) / 2 + 0.07])
        radial = verts.astype(np.float64) - centre
        assert np.all(np.einsum("ij,ij->i", got.astype(np.float64), radial) > 0), "normals point out of the sphere, toward lower values"
    # an anisotropic lattice: 1 / step scales the differences
    _normals_check(field, verts, inv_step=np.array([200.0, 100.0, 400.0], dtype=np.float32), label=name + " anisotropic")


def test_normals_at_arbitrary_points_and_in_flat_regions():
    field = mc.torus_field()
    rng = np.random.default_rng(12)
    v, _ = mc.marching_cubes_np(field, 0.02)
    # non-edge points: the surface's vertices pushed off their edges, inside the band where the field varies
    pts = (v + rng.uniform(-0.45, 0.45, v.shape)).astype(np.float32)
    _normals_check(field, pts, label="off-edge points")
    # the cube's corners and beyond-the-end coordinates: indices clamp, nothing is read outside
    n = field.shape[0]
    edge = np.array([[0, 0, 0], [n - 1, n - 1, n - 1], [n - 1, 0, n - 1], [0.5, n - 1, 0.25]], dtype=np.float32)
    flat = np.concatenate([edge, rng.uniform(0, 3, (64, 3)).astype(np.float32)])         # the field is 0 near the corner: flat
    got = F.mesh_normals(torch.from_numpy(field).to(DEV), torch.from_numpy(flat).to(DEV)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32) & 0x7FFFFFFF, np.zeros_like(got, dtype=np.uint32)), "a flat region gives exact zeros"
    empty = F.mesh_normals(torch.from_numpy(field).to(DEV), torch.empty((0, 3), device=DEV))
    assert empty.shape == (0, 3)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def renderers():
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
    hip_demo = importlib.import_module("hip_demo_render")
    z, meta = load("mesh/mesh_body")
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
    make = lambda **kw: R.Renderer(plain.encoder, plain.nerfhead, neg_ray_train=plain.neg_ray_train, neg_ray_val=plain.neg_ray_val,
                                   n_rays=plain.n_rays, n_samples=plain.n_samples, voxel_size=cfg.dataset.voxel_size, mesh_th=plain.mesh_th,
                                   progressive=True, **kw).to(DEV).eval()
    keys = ("src_imgs", "src_Ks", "src_poses", "feature", "coord", "out_sh", "bounds", "Rh", "R", "Th")
    b = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(DEV) for k in keys}
    b["featmaps"] = torch.from_numpy(sc["featmaps"]).to(DEV)
    b["volumes"] = [torch.from_numpy(v).to(DEV) for v in sc["volumes"]]
    b["target_K"] = torch.from_numpy(sc["target_K"]).to(DEV)
    b["target_pose"] = torch.from_numpy(sc["target_pose"]).to(DEV)
    with torch.no_grad():
        base = plain.render_mesh(b)
        coloured = make(mesh_colors=True).render_mesh(b)
        full = make(mesh_clean="largest", mesh_normals=True, mesh_colors=True).render_mesh(b)
    return NS(base=base, coloured=coloured, full=full, voxel=np.asarray(cfg.dataset.voxel_size, dtype=np.float64))


def test_render_mesh_with_every_option_off_is_todays(renderers):
    base = renderers.base
    rv, rf = mc.marching_cubes_np(base["cube"], ISO)
    assert np.array_equal(base["mesh"].vertices, rv.astype(np.float64)) and np.array_equal(base["mesh"].faces, rf)
    assert base["mesh"].vertex_normals is None and base["mesh"].vertex_colors is None and "mesh_stats" not in base


def test_render_mesh_cleans_colours_and_shades(renderers):
    base, coloured, full = renderers.base, renderers.coloured, renderers.full
    assert np.array_equal(full["cube"].view(np.uint32), base["cube"].view(np.uint32)), "the returned cube stays the untouched one"
    out, _, stats = cc.clean_np(base["cube"], ISO, cc.KEEP | cc.FILL, 0)
    assert full["mesh_stats"] == dict(zip(L.CUBE_STATS, stats.tolist())) and stats[0] > 1
    rv, rf = mc.marching_cubes_np(out, ISO)
    m = full["mesh"]
    assert np.array_equal(m.vertices, rv.astype(np.float64)) and np.array_equal(m.faces, rf)
    assert 0 < len(m.faces) < len(base["mesh"].faces) and cc.surfaces(m.faces, len(m.vertices)) == 1
    # colours: the plain coloured mesh's at the same vertex positions (a vertex of the cleaned mesh is one of the unfiltered mesh's)
    rows = lambda v: [r.tobytes() for r in np.ascontiguousarray(v, dtype=np.float32)]
    index = {k: i for i, k in enumerate(rows(coloured["mesh"].vertices))}
    pos = np.array([index[k] for k in rows(m.vertices)])
    assert np.array_equal(coloured["mesh"].vertices[pos], m.vertices)
    assert np.array_equal(coloured["mesh"].vertex_colors[pos].view(np.uint32), m.vertex_colors.view(np.uint32))
    # normals: of the cleaned cube, scaled by 1 / voxel size
    inv = (np.float32(1.0) / renderers.voxel.astype(np.float32)).astype(np.float32)
    n64, len64 = cc.normals_np(out, rv, inv, np.float64)
    n32, _ = cc.normals_np(out, rv, inv, np.float32)
    ok = len64 >= 1e-3 * float(np.abs(out).max()) * float(inv.min())
    d32 = float(np.abs(n32.astype(np.float64) - n64)[ok].max())
    dev = float(np.abs(m.vertex_normals.astype(np.float64) - n64)[ok].max())
    print(f"render_mesh normals: {len(rv)} vertices, {int((~ok).sum())} weak, d32 {d32:.3e}, device {dev:.3e}")
    assert m.vertex_normals.dtype == np.float32 and np.all(np.isfinite(m.vertex_normals)) and dev <= 4 * d32
    buf = __import__("io").BytesIO()
    m.export(buf)
    assert b"property float nx" in buf.getvalue()[:400] and b"property uchar red" in buf.getvalue()[:400]
