"""GPU: quadric vertex clustering (gpnerf_simplify.hip) against the numpy restatement of include/gpnerf_hip.h (tests/simplify_cases.py):
stats, faces (values and order), vertex_map and the number and order of vertices EQUAL, positions within one float32 ulp per
coordinate (both sides spell the same float64 operations in the same order, so bit equality is expected and the share of coordinates
that differ is printed); two runs and a graph replay identical; the size check of emit; extract_mesh(simplify=) and
Renderer(mesh_simplify=) end to end.

Measured on an MI355X: 0 of the 7 578 coordinates of the 18 cases were not bit-equal."""
import ctypes as C
import functools
import importlib
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import mesh_cases as mc
import simplify_cases as sc
from golden_cases import load, scene_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = importlib.import_module("gp-nerf_amd.frame")
R = importlib.import_module("gp-nerf_amd.render")
L = importlib.import_module("gp-nerf_amd._lib")
DEV = "cuda:0"
UNIT = ((0.0, 0.0, 0.0), 1.0)


def _swapped(mesh):
    v, f = mesh
    return v, np.ascontiguousarray(f[::-1])


def _auto(mesh, cell):
    v, f = mesh
    lo, cells = sc.auto_grid(v, cell)
    return v, f, lo, cell, cells


def _sparse():
    """three far-apart corners in a grid of 2^26 cells: sparse occupancy, the scan at its largest"""
    v = np.array([[0.5, 0.5, 0.5], [300.5, 200.25, 100.125], [511.5, 511.5, 255.5]], dtype=np.float32)
    return v, np.array([[0, 1, 2]], dtype=np.int32), (0.0, 0.0, 0.0), 1.0, (512, 512, 256)


TABLE = {
    "triangle_three_cells": lambda: (*sc.one_triangle(), *UNIT, (2, 2, 1)),
    "triangle_one_cell": lambda: (*sc.one_triangle(), (0.0, 0.0, 0.0), 2.0, (1, 1, 1)),
    "same_orientation": lambda: (*sc.coincident((1, 1)), *UNIT, (2, 2, 1)),
    "same_orientation_swapped": lambda: (*_swapped(sc.coincident((1, 1))), *UNIT, (2, 2, 1)),
    "opposite": lambda: (*sc.coincident((1, -1)), *UNIT, (2, 2, 1)),
    "three_net_plus": lambda: (*sc.coincident((1, -1, 1)), *UNIT, (2, 2, 1)),
    "three_net_minus": lambda: (*sc.coincident((-1, 1, -1)), *UNIT, (2, 2, 1)),
    "bad_faces": lambda: (*sc.bad_faces(), *UNIT, (4, 4, 4)),
    "flat_sheet": lambda: (*sc.flat_sheet(), *UNIT, (9, 9, 3)),
    "sphere_1.0": lambda: _auto(sc.mc_sphere(), 1.0),
    "sphere_2.0": lambda: _auto(sc.mc_sphere(), 2.0),
    "sphere_2.5": lambda: _auto(sc.mc_sphere(), 2.5),
    "torus_2.5": lambda: _auto(sc.mc_torus(), 2.5),
    "icosphere_2.0": lambda: _auto(sc.ico5(), 2.0),
    "fan": lambda: (*sc.fan(3000), *UNIT, (5, 5, 5)),
    "fan_shuffled": lambda: (*sc.fan(3000, shuffled=True), *UNIT, (5, 5, 5)),
    "sparse_2^26_cells": _sparse,
    "one_cell_grid": lambda: (*sc.mc_sphere(), (-1.0, -1.0, -1.0), 64.0, (1, 1, 1)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, lo, cell, cells, the restatement's result); built once and left unchanged"""
    v, f, lo, cell, cells = TABLE[name]()
    return v, f, lo, cell, cells, sc.simplify_np(v, f, lo, cell, cells)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def device_result(name):
    v, f, lo, cell, cells, _ = case(name)
    ov, of, stats, vmap = F.simplify_mesh(dev(v), dev(f), cell, lo=lo, cells=cells, want_map=True)
    torch.cuda.synchronize()
    return ov.cpu().numpy(), of.cpu().numpy(), stats.cpu().numpy(), vmap.cpu().numpy()


BITS = {"coordinates": 0, "differing": 0}


@pytest.mark.parametrize("name", list(TABLE))
def test_simplify_is_the_restatement(name):
    v, f, lo, cell, cells, ref = case(name)
    ov, of, stats, vmap = device_result(name)
    print(name, dict(zip(L.SIMPLIFY_STATS, stats.tolist())))
    assert stats.dtype == np.int64 and stats.tolist() == sc.stats_row(ref["stats"])
    assert of.dtype == np.int32 and of.shape == ref["faces"].shape and np.array_equal(of, ref["faces"])
    assert vmap.dtype == np.int32 and np.array_equal(vmap, ref["vertex_map"])
    assert ov.dtype == np.float32 and ov.shape == ref["vertices"].shape
    diff = np.abs(ov.astype(np.float64) - ref["vertices"].astype(np.float64))
    differing = int((ov.view(np.uint32) != ref["vertices"].view(np.uint32)).sum()) if ov.size else 0
    BITS["coordinates"] += ov.size
    BITS["differing"] += differing
    print(f"{name}: {len(ov)} vertices, {len(of)} faces, {differing} of {ov.size} coordinates not bit-equal, largest difference "
          f"{float(diff.max()) if ov.size else 0.0:.3e}; so far {BITS['differing']} of {BITS['coordinates']}")
    assert np.all(diff <= sc.position_tolerance(ref["vertices"], lo, cell, cells))


def test_the_cases_reach_their_branches():
    row = lambda name: dict(zip(L.SIMPLIFY_STATS, device_result(name)[2].tolist()))
    assert row("triangle_three_cells")["faces_out"] == 1 and row("triangle_three_cells")["vertices_out"] == 3
    one = row("triangle_one_cell")
    assert (one["vertices_out"], one["faces_out"], one["faces_collapsed"], one["clusters_dropped"]) == (0, 0, 1, 1)
    assert device_result("triangle_one_cell")[0].shape == (0, 3) and device_result("triangle_one_cell")[1].shape == (0, 3)
    assert device_result("triangle_one_cell")[3].tolist() == [-1, -1, -1]
    for name in ("same_orientation", "same_orientation_swapped"):
        assert row(name)["faces_duplicate"] == 1 and row(name)["faces_out"] == 1
    # the kept one is the lower index in either input order: its corner order is that of the first row
    assert device_result("same_orientation")[1].tolist() == [[0, 2, 1]] and device_result("same_orientation_swapped")[1].tolist() == [[0, 2, 1]]
    opp = row("opposite")
    assert (opp["faces_cancelled"], opp["faces_out"], opp["vertices_out"], opp["clusters_dropped"]) == (2, 0, 0, 3)
    assert row("three_net_plus")["faces_cancelled"] == 2 and device_result("three_net_plus")[1].tolist() == [[0, 2, 1]]
    assert row("three_net_minus")["faces_cancelled"] == 2 and device_result("three_net_minus")[1].tolist() == [[0, 1, 2]]
    bad = row("bad_faces")
    assert (bad["faces_invalid"], bad["faces_out"], bad["vertices_out"]) == (10, 2, 6)
    ov, of = device_result("bad_faces")[:2]
    assert ov[of[1]].tolist() == [[0.5, 2.5, 2.5], [1.5, 2.5, 2.5], [2.5, 2.5, 2.5]]      # the zero-area face: no quadric, the centres
    assert row("sphere_2.5")["faces_cancelled"] == 2 and row("sphere_2.5")["clusters_dropped"] == 1 and row("sphere_2.5")["clusters_clamped"] > 0
    assert row("sparse_2^26_cells")["vertices_out"] == 3
    assert row("one_cell_grid")["faces_collapsed"] == 3784 and row("one_cell_grid")["vertices_out"] == 0
    for name, chi in (("sphere_2.0", 2), ("sphere_2.5", 2), ("torus_2.5", 0), ("icosphere_2.0", 2)):
        ov, of = device_result(name)[:2]
        assert mc.euler_and_closed(ov, of.astype(np.int64)) == (chi, True, True), name


def test_a_flat_sheet_stays_flat_on_the_device():
    ov = device_result("flat_sheet")[0].astype(np.float64)
    h, cell, n = 1.3, 1.0, 9
    assert len(ov) == n * n
    assert np.abs(ov[:, 2] - np.float32(h)).max() <= (sc.EPS / 3.0) * (cell / 2.0) + 2.0 ** -23 * h
    centres = (np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2) + 0.5) * cell
    assert np.array_equal(ov[:, :2], centres)


def test_a_list_far_longer_than_a_wavefront_does_not_depend_on_the_face_order():
    """the fan's centre cluster holds all 3000 faces.  Ascending and shuffled input: the same clusters and the same set of kept
    triangles; the two quadrics are summed in the order of the face indices each run was given, so the centre may differ by a
    rounding of the final cast and nothing else may."""
    (va, fa, lo, cell, cells, _), (vs, fs, *_rest) = case("fan"), case("fan_shuffled")
    a, s = device_result("fan"), device_result("fan_shuffled")
    assert np.array_equal(va, vs) and sorted(map(tuple, fa.tolist())) == sorted(map(tuple, fs.tolist()))
    assert a[2].tolist() == s[2].tolist() and np.array_equal(a[3], s[3]) and a[2][1] > 8
    assert sorted(map(tuple, a[1].tolist())) == sorted(map(tuple, s[1].tolist()))
    assert np.all(np.abs(a[0].astype(np.float64) - s[0]) <= sc.position_tolerance(a[0], lo, cell, cells))
    # and in one order, run to run, the bits are the same whatever order the lists were filled in
    again = F.simplify_mesh(dev(vs), dev(fs), cell, lo=lo, cells=cells)[0].cpu().numpy()
    assert again.tobytes() == s[0].tobytes()


def test_vertex_map_and_the_distance_bound_on_the_device_result():
    for name in ("sphere_1.0", "sphere_2.5", "torus_2.5", "fan", "bad_faces"):
        v, f, lo, cell, cells, ref = case(name)
        ov, of, stats, vmap = device_result(name)
        used = np.unique(f[ref["valid"]].reshape(-1))
        mapped = used[vmap[used] >= 0]
        assert len(mapped) and vmap.max() == len(ov) - 1
        d = np.linalg.norm(v[mapped].astype(np.float64) - ov[vmap[mapped]].astype(np.float64), axis=1)
        span = float(np.abs(np.asarray(lo, dtype=np.float64)).max() + max(cells) * cell)
        print(f"{name}: largest distance to the cluster's position {d.max() / cell:.3f} cells")
        assert d.max() <= math.sqrt(3.0) * cell + 8 * 2.0 ** -23 * span


def _raw(name, n_out=None):
    """the two entry points on buffers of the test's own: (run, buffers)"""
    v, f, lo, cell, cells, ref = case(name)
    lib = L.lib()
    tv, tf = dev(v), dev(f)
    c_lo, c_cells = (C.c_float * 3)(*[float(x) for x in lo]), (C.c_int32 * 3)(*cells)
    ws = torch.zeros((int(lib.gpnerf_mesh_simplify_workspace_bytes(len(v), len(f), c_cells)),), device=DEV, dtype=torch.uint8)
    nv, nf = n_out if n_out is not None else (ref["stats"]["vertices_out"], ref["stats"]["faces_out"])
    b = NS(ws=ws, stats=torch.zeros((8,), device=DEV, dtype=torch.int64), ov=torch.zeros((max(nv, 1), 3), device=DEV),
           of=torch.zeros((max(nf, 1), 3), device=DEV, dtype=torch.int32), vmap=torch.zeros((len(v),), device=DEV, dtype=torch.int32))

    def run(count=True):
        st = F._stream_ptr(torch.device(DEV))
        if count:
            L.check(lib.gpnerf_mesh_simplify_count(tv.data_ptr(), len(v), tf.data_ptr(), len(f), c_lo, cell, c_cells, ws.data_ptr(), ws.numel(),
                                                   b.stats.data_ptr(), st), "count")
        return lib.gpnerf_mesh_simplify_emit(tv.data_ptr(), len(v), tf.data_ptr(), len(f), ws.data_ptr(), ws.numel(), nv, nf, b.ov.data_ptr(),
                                             b.of.data_ptr(), b.vmap.data_ptr(), st)
    return run, b


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    name = "torus_2.5"
    run, b = _raw(name)
    outs = lambda: [t.cpu().numpy().tobytes() for t in (b.stats, b.ov, b.of, b.vmap)]
    assert run() == 0                                       # (also loads the kernels before the capture)
    torch.cuda.synchronize()
    first = outs()
    ref = device_result(name)
    assert first[1] == ref[0].tobytes() and first[2] == ref[1].tobytes() and first[3] == ref[3].tobytes()
    assert run() == 0
    torch.cuda.synchronize()
    assert outs() == first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert run() == 0
    for _ in range(2):
        for t in (b.stats, b.ov, b.of, b.vmap):
            t.fill_(7)                                      # every output is written by the calls
        b.ws.fill_(0xAB)                                    # the workspace carries nothing into a call
        g.replay()
        torch.cuda.synchronize()
        assert outs() == first


def test_emit_checks_the_sizes_on_the_device():
    name = "sphere_2.0"
    ref = case(name)[5]["stats"]
    status = lambda b: int(b.ws[:256].view(torch.int64)[L.SIMPLIFY_HDR_STATUS].item())
    run, b = _raw(name, n_out=(ref["vertices_out"], ref["faces_out"] - 1))
    for t in (b.ov, b.of, b.vmap):
        t.fill_(7)
    assert run() == 0                                       # the host cannot know; nothing is read back
    torch.cuda.synchronize()
    assert status(b) == L.SIMPLIFY_MISMATCH
    assert all(bool((t == 7).all()) for t in (b.ov, b.of, b.vmap)), "a mismatched emit writes nothing"
    run, b = _raw(name)
    assert run() == 0
    torch.cuda.synchronize()
    assert status(b) == L.SIMPLIFY_EMITTED and np.array_equal(b.of.cpu().numpy(), device_result(name)[1])
    b.ws[:256].fill_(0)                                     # no finished count in the workspace
    b.of.fill_(7)
    assert run(count=False) == 0
    torch.cuda.synchronize()
    assert bool((b.of == 7).all())


def test_the_box_is_taken_from_the_vertices_when_no_grid_is_given():
    v, f = sc.mc_sphere()
    lo, cells = F.simplify_grid(v.min(0), v.max(0), 2.0)
    ov, of, stats, vmap = F.simplify_mesh(dev(v), dev(f), 2.0)
    ref = sc.simplify_np(v, f, lo, 2.0, cells)
    assert vmap is None and stats.cpu().tolist() == sc.stats_row(ref["stats"]) and np.array_equal(of.cpu().numpy(), ref["faces"])
    assert mc.euler_and_closed(ov.cpu().numpy(), of.cpu().numpy().astype(np.int64)) == (2, True, True)
    empty = F.simplify_mesh(torch.empty((0, 3), device=DEV), torch.empty((0, 3), device=DEV, dtype=torch.int32), 1.0, want_map=True)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].cpu().tolist() == [0] * 8 and empty[3].shape == (0,)
    with pytest.raises(L.GpnerfError):
        F.simplify_mesh(dev(v), dev(f), 0.0)
    with pytest.raises(L.GpnerfError):
        F.simplify_mesh(dev(v), dev(f), 0.001, lo=(0, 0, 0), cells=(4096, 4096, 4096))
    with pytest.raises(L.GpnerfError):
        F.simplify_mesh(dev(v), dev(f.astype(np.int64)), 1.0)


def test_extract_mesh_simplifies_behind_marching_cubes():
    """the sphere cube through the lattice= route: the simplified mesh is the restatement's on marching cubes' mesh with lo = -1/2
    and cells = ceil(dim / k) + 1; normals are taken at the new vertices"""
    field = mc.sphere_field(32, 10.0)
    cube = torch.from_numpy(field).to(DEV)
    axes = [np.arange(32, dtype=np.float32) * np.float32(0.005)] * 3
    n_kept = torch.zeros((), device=DEV, dtype=torch.int64)
    vs = np.array([0.005, 0.005, 0.005])
    plain = F.extract_mesh(None, None, None, None, None, iso=0.02, host=[vs], lattice=(cube, axes, n_kept))
    assert "simplify_stats" not in plain and plain["faces"].shape[0] == 3784
    for off in (None, 0, "0", ""):
        assert "simplify_stats" not in F.extract_mesh(None, None, None, None, None, iso=0.02, host=[vs], lattice=(cube, axes, n_kept), simplify=off)
    m = F.extract_mesh(None, None, None, None, None, iso=0.02, host=[vs], lattice=(cube, axes, n_kept), normals=True, simplify=2)
    torch.cuda.synchronize()
    v, f = sc.mc_sphere()
    ref = sc.simplify_np(v, f, (-0.5, -0.5, -0.5), 2.0, (17, 17, 17))
    assert m["simplify_stats"].cpu().tolist() == sc.stats_row(ref["stats"]) and np.array_equal(m["faces"].cpu().numpy(), ref["faces"])
    ov, n = m["vertices"].cpu().numpy(), m["normals"].cpu().numpy()
    assert ov.shape == ref["vertices"].shape == n.shape and 0 < len(ov) < len(v) / 3
    assert np.all(np.abs(ov.astype(np.float64) - ref["vertices"]) <= sc.position_tolerance(ref["vertices"], (-0.5,) * 3, 2.0, (17,) * 3))
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-5
    centre = np.array([15.5 + 0.31, 15.5 - 0.17, 15.5 + 0.07])
    radial = (ov - centre) / np.linalg.norm(ov - centre, axis=1, keepdims=True)
    assert (np.sum(radial * n, axis=1) > 0.9).all()         # outward: toward lower values
    assert mc.euler_and_closed(ov, m["faces"].cpu().numpy().astype(np.int64)) == (2, True, True)


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
    scn = scene_of(meta)
    cfg = NS(encoder=NS(file="fixed_encoder", name="resnet34", out_ch=32),
             head=NS(file="hip_head", rgb=NS(use_rgbhead=False),
                     sigma=NS(code_dim=32, n_heads=4, n_layers=4, n_smpl=6890, outdims=[32, 32, 32, 32])),
             dataset=NS(train=NS(name="zju_mocap", chunk=400), test=NS(name="zju_mocap", chunk=2000),
                        voxel_size=[float(x) for x in scn["voxel_size"]]),
             train=NS(n_rays=1024, n_samples=32), test=NS(mesh_th=50))
    plain = hip_demo.build_render(cfg).to(DEV).eval()
    sd = plain.state_dict()
    for k, v in scn["head"].items():
        sd["nerfhead." + k] = torch.from_numpy(v.copy())
    plain.load_state_dict(sd, strict=True)
    make = lambda **kw: R.Renderer(plain.encoder, plain.nerfhead, neg_ray_train=plain.neg_ray_train, neg_ray_val=plain.neg_ray_val,
                                   n_rays=plain.n_rays, n_samples=plain.n_samples, voxel_size=cfg.dataset.voxel_size, mesh_th=plain.mesh_th,
                                   progressive=True, **kw).to(DEV).eval()
    keys = ("src_imgs", "src_Ks", "src_poses", "feature", "coord", "out_sh", "bounds", "Rh", "R", "Th")
    b = {k: torch.from_numpy(np.ascontiguousarray(scn[k])).to(DEV) for k in keys}
    b["featmaps"] = torch.from_numpy(scn["featmaps"]).to(DEV)
    b["volumes"] = [torch.from_numpy(v).to(DEV) for v in scn["volumes"]]
    b["target_K"] = torch.from_numpy(scn["target_K"]).to(DEV)
    b["target_pose"] = torch.from_numpy(scn["target_pose"]).to(DEV)
    with torch.no_grad():
        base = plain.render_mesh(b)
        off = make(mesh_simplify=0).render_mesh(b)
        simple = make(mesh_simplify=2, mesh_normals=True, mesh_colors=True).render_mesh(b)
        both = make(mesh_simplify="2", mesh_clean="largest").render_mesh(b)
    return NS(base=base, off=off, simple=simple, both=both)


def test_render_mesh_with_the_knob_off_is_todays(renderers):
    base, off = renderers.base, renderers.off
    assert set(off) == set(base) == {"mesh", "cube", "time_slots", "etime", "rtime"}
    assert np.array_equal(off["mesh"].vertices, base["mesh"].vertices) and np.array_equal(off["mesh"].faces, base["mesh"].faces)


def test_render_mesh_simplifies_colours_and_shades(renderers):
    base, simple, both = renderers.base, renderers.simple, renderers.both
    s = simple["mesh_stats"]
    assert list(s) == list(L.SIMPLIFY_STATS)
    assert list(both["mesh_stats"]) == list(L.CUBE_STATS) + list(L.SIMPLIFY_STATS)
    m = simple["mesh"]
    print("render_mesh(mesh_simplify=2):", len(base["mesh"].faces), "faces ->", s)
    assert (len(m.vertices), len(m.faces)) == (s["vertices_out"], s["faces_out"]) and 0 < len(m.faces) < len(base["mesh"].faces) / 2
    assert len(base["mesh"].faces) == s["faces_out"] + s["faces_invalid"] + s["faces_collapsed"] + s["faces_cancelled"] + s["faces_duplicate"]
    assert s["faces_invalid"] == 0 and m.faces.min() == 0 and m.faces.max() == len(m.vertices) - 1
    assert m.vertex_colors.shape == m.vertices.shape == m.vertex_normals.shape
    assert np.isfinite(m.vertex_colors).all() and m.vertex_colors.min() >= 0.0 and m.vertex_colors.max() <= 1.0
    norms = np.linalg.norm(m.vertex_normals.astype(np.float64), axis=1)
    assert np.isfinite(m.vertex_normals).all() and np.abs(norms[norms > 0.5] - 1.0).max() < 1e-5 and (norms > 0.5).mean() > 0.99
    # the restatement on the plain mesh, with extract_mesh's grid
    cube = base["cube"]
    ref = sc.simplify_np(base["mesh"].vertices.astype(np.float32), base["mesh"].faces, (-0.5, -0.5, -0.5), 2.0,
                         [int(math.ceil(d / 2.0)) + 1 for d in cube.shape])
    assert sc.stats_row(ref["stats"]) == [s[k] for k in L.SIMPLIFY_STATS] and np.array_equal(m.faces, ref["faces"])
    print("render_mesh(mesh_simplify=2):", int((m.vertices.astype(np.float32).view(np.uint32) != ref["vertices"].view(np.uint32)).sum()), "of",
          ref["vertices"].size, "coordinates not bit-equal to the restatement")
    assert np.all(np.abs(m.vertices - ref["vertices"]) <= sc.position_tolerance(ref["vertices"], (-0.5,) * 3, 2.0, [d / 2.0 + 1 for d in cube.shape]))
    buf = __import__("io").BytesIO()
    m.export(buf)
    assert len(buf.getvalue()) > 0
