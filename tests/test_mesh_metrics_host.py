"""CPU: the mesh-evaluation restatements pinned on analytic cases (tests/mesh_metric_cases.py), every host-side refusal of the four new
entry points (they are refused before any device call, so no GPU is needed), the workspace arithmetic, load_mesh and
Mesh.to_lattice_frame."""
import ctypes as C
import importlib
import io
import math
import os

import numpy as np
import pytest
import torch

import mesh_metric_cases as mm

M = importlib.import_module("gp-nerf_amd.mesh")
L = importlib.import_module("gp-nerf_amd._lib")
F = importlib.import_module("gp-nerf_amd.frame")
P = 0x1000                                  # a non-null pointer that is never dereferenced: every call below is refused on the host


def test_the_restatement_on_a_unit_right_triangle():
    v, f = mm.one_triangle()
    a, b, c = v[0], v[1], v[2]

    def one(p):
        cp, d, region = mm.closest_on_triangle(np.array(p, np.float64), a, b, c)
        return cp + np.array(p), float(d), mm.REGIONS[int(region)]

    cp, d, r = one([0.25, 0.25, 0.5])                                      # above the interior
    assert r == "interior" and d == 0.5 and np.allclose(cp, [0.25, 0.25, 0])
    cp, d, r = one([0.5, -0.25, 0.0])                                      # beside each edge
    assert r == "edge_ab" and d == 0.25 and np.allclose(cp, [0.5, 0, 0])
    cp, d, r = one([-0.5, 0.5, 0.0])
    assert r == "edge_ca" and d == 0.5 and np.allclose(cp, [0, 0.5, 0])
    cp, d, r = one([1.0, 1.0, 0.0])
    assert r == "edge_bc" and abs(d - math.sqrt(0.5)) < 1e-15 and np.allclose(cp, [0.5, 0.5, 0])
    cp, d, r = one([-0.375, -0.5, 0.0])                                    # beyond each vertex (inputs are rounded to float32: dyadic)
    assert r == "vertex_a" and d == 0.625
    cp, d, r = one([2.0, -0.5, 0.0])
    assert r == "vertex_b" and abs(d - math.hypot(1.0, 0.5)) < 1e-15 and np.allclose(cp, [1, 0, 0])
    cp, d, r = one([-0.5, 3.0, 1.0])
    assert r == "vertex_c" and abs(d - math.sqrt(0.25 + 4 + 1)) < 1e-15 and np.allclose(cp, [0, 1, 0])
    for p in ([0, 0, 0], [0.5, 0.5, 0], [0.25, 0.25, 0]):                  # on a vertex, on an edge, in the plane
        assert one(p)[1] == 0.0


def test_the_restatement_on_degenerate_triangles():
    seg = (np.array([0.0, 0, 0]), np.array([2.0, 0, 0]), np.array([1.0, 0, 0]))         # collinear: the segment (0,0,0)-(2,0,0)
    for p, want in (([1.0, 1.0, 0], 1.0), ([3.0, 0, 0], 1.0), ([-1.0, 0, 1.0], math.sqrt(2.0)), ([1.5, 0, 0], 0.0)):
        cp, d, r = mm.closest_on_triangle(np.array(p), *seg)
        assert mm.REGIONS[int(r)] == "degenerate" and abs(float(d) - want) < 1e-15
    pt = np.array([0.5, 0.5, 0.5])
    cp, d, r = mm.closest_on_triangle(np.array([0.5, 0.5, 2.5]), pt, pt, pt)
    assert mm.REGIONS[int(r)] == "degenerate" and float(d) == 2.0
    for dtype in (np.float32, np.float64):
        v, f = mm.degenerate_mix()
        d = mm.all_distances(mm.degenerate_queries(), v, f, dtype)
        assert np.isfinite(d).all()


def test_concentric_cubes_are_at_the_known_offset():
    """every sample on a face of the inner cube (half 1) is 0.25 from the outer one (half 1.25), and the reverse but for the rounded
    edges: a point of an outer face over the inner face's interior is at 0.25 too"""
    vi, fi = mm.cube_mesh(1.0)
    vo, fo = mm.cube_mesh(1.25)
    rng = np.random.default_rng(1)
    pts = []
    for axis in range(3):
        for side in (-1.0, 1.0):
            p = rng.uniform(-1, 1, (50, 3))
            p[:, axis] = side
            pts.append(p)
    pts = mm.f32(np.concatenate(pts))
    d, _ = mm.nearest(pts, vo, fo)
    assert np.abs(d - 0.25).max() < 1e-15
    d, _ = mm.nearest(mm.f32(pts * np.where(np.abs(pts) == 1.0, 1.25, 1.0)), vi, fi)
    assert np.abs(d - 0.25).max() < 1e-15


def test_every_region_is_reached_by_the_constructed_queries():
    for v, f in (mm.one_triangle(), mm.two_triangles()):
        q = mm.region_queries(v, f, 1000)
        for tri in f:
            _, d, region = mm.closest_on_triangle(q, v[tri[0]], v[tri[1]], v[tri[2]])
            assert set(np.unique(region)) == set(range(1, 8)), np.unique(region)
            assert (d == 0).sum() >= 3
    assert [len(mm.region_queries(*mm.one_triangle(), n)) for n in (1, 63, 64, 65, 1000)] == [1, 63, 64, 65, 1000]


def test_the_tie_queries_are_bit_equal_ties_in_float32():
    v, f = mm.tie_cube()
    d = mm.all_distances(mm.tie_queries(), v, f, np.float32)
    assert d.dtype == np.float32
    ties = d == d.min(axis=1, keepdims=True)
    assert (ties.sum(axis=1) >= 2).all()
    owners = {tuple(np.nonzero(t)[0] // 2) for t in ties}                 # quads: +x is 0, +y is 5
    assert owners <= {(0, 5), (0, 0, 5), (0, 5, 5), (0, 0, 5, 5)} and len(v) == 24 and len(f) == 12


def test_the_hash_is_murmur3s_finalizer():
    """fmix32 restated once more, as Python integers, and three of its published-constant values"""
    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85ebca6b) & 0xffffffff
        h ^= h >> 13
        h = (h * 0xc2b2ae35) & 0xffffffff
        return h ^ (h >> 16)

    xs = [0, 1, 2, 0xdeadbeef, 0xffffffff, 12345]
    assert [int(x) for x in mm.fmix32(np.array(xs, np.uint32))] == [fmix(x) for x in xs]
    assert fmix(0) == 0 and fmix(1) == 0x514e28b7
    r1, r2 = mm.sample_randoms(7, np.arange(10))
    assert [float(x) for x in r1] == [(fmix(7 ^ fmix(2 * i)) >> 8) / 2.0 ** 24 for i in range(10)]
    assert [float(x) for x in r2] == [(fmix(7 ^ fmix(2 * i + 1)) >> 8) / 2.0 ** 24 for i in range(10)]
    assert ((r1 >= 0) & (r1 < 1)).all()


def test_icospheres_have_the_sizes_the_gpu_cases_name():
    for level, nf in ((2, 320), (3, 1280)):
        v, f = mm.icosphere(level)
        assert f.shape == (nf, 3) and np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1).max() < 1e-6
        assert 0 < 4 * math.pi - mm.face_areas(v, f).sum() < 4 * math.pi * (0.025 if level == 2 else 0.007)      # inscribed: a little less


def test_every_refusal_happens_on_the_host():
    lib = L.lib()
    E = -1
    ws_bytes = int(lib.gpnerf_mesh_grid_workspace_bytes(10, 64, 100))
    assert ws_bytes > 0

    def build(vertices=P, n_vertices=8, faces=P, n_faces=10, cell_cap=64, entry_cap=100, ws=P, nbytes=ws_bytes):
        return lib.gpnerf_mesh_grid_build(vertices, n_vertices, faces, n_faces, cell_cap, entry_cap, ws, nbytes, None)

    assert build(vertices=None) == E and build(faces=None) == E and build(ws=None) == E
    assert build(n_vertices=-1) == E and build(n_faces=0) == E and build(n_faces=-3) == E and build(n_faces=1 << 31) == E
    assert build(cell_cap=0) == E and build(entry_cap=0) == E and build(cell_cap=-1) == E and build(entry_cap=-1) == E
    assert build(nbytes=ws_bytes - 1) == E and build(nbytes=0) == E
    for args in ((0, 64, 100), (-1, 64, 100), (10, 0, 100), (10, 64, 0), (10, (1 << 24) + 1, 100), (10, 64, (1 << 30) + 1), (1 << 31, 64, 100)):
        assert lib.gpnerf_mesh_grid_workspace_bytes(*args) == 0, args

    def distance(points=P, n_points=4, vertices=P, n_vertices=8, faces=P, n_faces=10, grid=None, max_dist=math.inf, normals=None, dist=P,
                 face=P, closest=None, cosine=None):
        return lib.gpnerf_mesh_distance(points, n_points, vertices, n_vertices, faces, n_faces, grid, max_dist, normals, dist, face, closest,
                                        cosine, None)

    assert distance(points=None) == E and distance(vertices=None) == E and distance(faces=None) == E and distance(dist=None) == E
    assert distance(face=None) == E and distance(n_points=-1) == E and distance(n_faces=0) == E and distance(n_vertices=-1) == E
    assert distance(max_dist=0.0) == E and distance(max_dist=-1.0) == E and distance(max_dist=math.nan) == E
    assert distance(normals=P) == E and distance(cosine=P) == E                  # one without the other
    assert distance(n_points=0) == 0 and distance(n_points=0, points=None, dist=None, face=None) == 0       # a no-op
    assert distance(n_points=0, max_dist=0.0) == E

    sbytes = int(lib.gpnerf_mesh_sample_workspace_bytes(10))
    assert sbytes >= 256 + 80 and lib.gpnerf_mesh_sample_workspace_bytes(0) == 0 and lib.gpnerf_mesh_sample_workspace_bytes(1 << 31) == 0

    def sample(vertices=P, n_vertices=8, faces=P, n_faces=10, n=5, ws=P, nbytes=sbytes, points=P):
        return lib.gpnerf_mesh_sample_surface(vertices, n_vertices, faces, n_faces, n, 0, ws, nbytes, points, None, None, None)

    assert sample(vertices=None) == E and sample(faces=None) == E and sample(ws=None) == E and sample(points=None) == E
    assert sample(n_vertices=-1) == E and sample(n_faces=0) == E and sample(n=-1) == E and sample(n=1 << 31) == E
    assert sample(nbytes=sbytes - 1) == E and sample(n=0, points=None) == 0

    th = (C.c_float * 4)(0.1, 0.2, 0.3, 0.4)
    stats = lambda values=P, n=5, t=th, nt=4, out=P: lib.gpnerf_distance_stats(values, n, t, nt, out, None)
    assert stats(values=None) == E and stats(out=None) == E and stats(n=-1) == E and stats(nt=5) == E and stats(nt=-1) == E
    assert stats(t=None) == E


def test_the_workspace_formula_and_the_default_capacities():
    lib = L.lib()
    a = int(lib.gpnerf_mesh_grid_workspace_bytes(1000, 1000, 10000))
    assert 8 * 1000 + 12 * 10000 + 33 * 1024 <= a <= 8 * 1000 + 12 * 10000 + 33 * 1024 + 8 * 256
    assert int(lib.gpnerf_mesh_grid_workspace_bytes(1, 1, 1)) > 256
    assert F.mesh_grid_caps(12) == (64, 8 * 12 + 4 * 64) and F.mesh_grid_caps(100000) == (100000, 1200000)
    assert F.mesh_grid_caps(1 << 25)[0] == 1 << 22
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpnerf_hip.h")).read()
    for name, word in L.GRID_HDR.items():
        assert f"#define GPNERF_GRID_HDR_{name.upper()} {word}\n" in hdr
    for name in ("FINITE", "INF", "NAN", "MEAN", "MEAN_SQ", "MAX", "WITHIN", "MAX_THRESHOLDS", "DOUBLES"):
        assert f"#define GPNERF_DIST_{name} {getattr(L, 'DIST_' + name)}\n" in hdr
    assert L.DIST_WITHIN + L.DIST_MAX_THRESHOLDS == L.DIST_DOUBLES


def test_cpu_tensors_are_refused():
    v, f = mm.one_triangle()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    for call in (lambda: F.build_mesh_grid(tv, tf), lambda: F.point_mesh_distance(torch.zeros(2, 3), tv, tf),
                 lambda: F.sample_surface(tv, tf, 4), lambda: F.distance_stats(torch.zeros(3)),
                 lambda: F.mesh_metrics((tv, tf), (tv, tf), device="cpu")):
        with pytest.raises(L.GpnerfError, match="no CPU fallback"):
            call()


def test_read_mesh_metrics_on_hand_made_slots():
    s = np.full((4, L.DIST_DOUBLES), np.nan)
    s[0, :6] = [90, 10, 0, 0.01, 0.0002, 0.05]
    s[1, :6] = [100, 0, 0, 0.03, 0.001, 0.08]
    s[0, L.DIST_WITHIN:L.DIST_WITHIN + 2] = [0.5, 0.9]
    s[1, L.DIST_WITHIN:L.DIST_WITHIN + 2] = [0.25, 0.0]
    s[2, L.DIST_MEAN], s[3, L.DIST_MEAN] = 0.8, 0.6
    r = F.read_mesh_metrics(s, thresholds=(0.01, 0.02))
    assert r["accuracy"] == 0.01 and r["completeness"] == 0.03 and r["chamfer"] == 0.02 and abs(r["normal_consistency"] - 0.7) < 1e-15
    assert r["precision@0.01"] == 0.5 and r["recall@0.01"] == 0.25 and abs(r["fscore@0.01"] - 2 * 0.5 * 0.25 / 0.75) < 1e-15
    assert r["fscore@0.02"] == 0.0 and r["accuracy_max"] == 0.05 and r["completeness_max"] == 0.08
    assert (r["n_pred"], r["beyond_pred"], r["nan_pred"], r["n_gt"]) == (90, 10, 0, 100)
    s[1, :3] = [0, 0, 100]
    with pytest.raises(L.GpnerfError, match="overflowed"):
        F.read_mesh_metrics(s, thresholds=(0.01, 0.02))


def test_to_lattice_frame_against_hand_arithmetic():
    axes = [np.array([-0.5, -0.25, 0.0, 0.25]), np.array([1.0, 1.5, 2.0]), np.array([0.0, 0.125])]       # steps 0.25, 0.5, 0.125
    m = M.Mesh([[10, 10, 10], [13, 12, 11], [11.5, 10.5, 10.25]], [[0, 1, 2]], vertex_colors=[[0, 0.5, 1]] * 3,
               vertex_normals=[[1, 0, 0], [0, 0, 0], [0.6, 0.8, 0]])
    t = m.to_lattice_frame(axes, 10)
    assert t is not m and t.vertices.dtype == np.float64
    assert t.vertices.tolist() == [[-0.5, 1.0, 0.0], [0.25, 2.0, 0.125], [-0.5 + 1.5 * 0.25, 1.0 + 0.5 * 0.5, 0.25 * 0.125]]
    assert np.array_equal(t.faces, m.faces) and np.array_equal(t.vertex_colors, m.vertex_colors)
    g = np.array([0.6 / 0.25, 0.8 / 0.5, 0.0])
    assert np.allclose(t.vertex_normals, [[1, 0, 0], [0, 0, 0], g / np.linalg.norm(g)], atol=1e-7)
    assert M.Mesh(m.vertices, m.faces).to_lattice_frame(axes, 10).vertex_normals is None
    assert np.array_equal(m.vertices[0], [10, 10, 10])                     # the original is untouched


@pytest.mark.parametrize("colours,normals", [(False, False), (True, False), (False, True), (True, True)])
def test_load_mesh_round_trips_what_export_writes(tmp_path, colours, normals):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(7, 3))
    f = rng.integers(0, 7, (9, 3))
    m = M.Mesh(v, f, rng.uniform(0, 1, (7, 3)) if colours else None, rng.normal(size=(7, 3)) if normals else None)
    path = tmp_path / "m.ply"
    m.export(str(path))
    back = M.load_mesh(str(path))
    assert back.vertices.tobytes() == m.vertices.tobytes() and np.array_equal(back.faces, m.faces)
    assert (back.vertex_normals is None) == (not normals) and (back.vertex_colors is None) == (not colours)
    if normals:
        assert back.vertex_normals.tobytes() == m.vertex_normals.tobytes()
    again = io.BytesIO()
    back.export(again)
    assert again.getvalue() == path.read_bytes()                           # bit for bit, the colour bytes included


def test_load_mesh_reads_float_ply_vertices(tmp_path):
    head = ("ply\nformat binary_little_endian 1.0\ncomment float xyz\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
            "element face 1\nproperty list uchar int vertex_indices\nend_header\n").encode()
    v = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25]], "<f4")
    path = tmp_path / "f.ply"
    path.write_bytes(head + v.tobytes() + b"\x03" + np.array([0, 1, 2], "<i4").tobytes())
    m = M.load_mesh(str(path))
    assert m.vertices.dtype == np.float64 and np.array_equal(m.vertices, v.astype(np.float64)) and m.faces.tolist() == [[0, 1, 2]]


def test_load_mesh_reads_an_obj_with_quads_slashes_and_negative_indices(tmp_path):
    text = """# a small fixture
mtllib none.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0.5 0.5
vn 0 0 1
f 1 2 3 4
v 0.5 0.5 1.5
f 1/1/1 2/1/1 5/1/1
f -1//1 -3//1 -2//1
f 2/1 3/1 -1/1
g ignored
"""
    path = tmp_path / "s.obj"
    path.write_text(text)
    m = M.load_mesh(str(path))
    assert m.vertices.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.5]]
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [4, 2, 3], [1, 2, 4]]
    assert m.vertex_colors is None and m.vertex_normals is None


def test_the_loop_leaves_a_gt_mesh_of_any_documented_form_whole():
    """evaluate_loop moves a batch's tensors to the device; a gt_mesh that is a Mesh or a pair of numpy arrays has nothing to move and
    must arrive as it is, a pair of tensors is moved element by element"""
    import types
    ev = importlib.import_module("gp-nerf_amd.evaluator")
    v, f = mm.one_triangle()
    seen = []

    class Keep:
        def evaluate(self, output, batch):
            seen.append(batch["gt_mesh"])

        def summarize(self):
            return {}

    class Render(torch.nn.Module):
        def render(self, batch):
            return {"rtime": 0.0}

    cfg = types.SimpleNamespace(test=types.SimpleNamespace(test_seq="s"), head=types.SimpleNamespace(rgb=types.SimpleNamespace(use_rgbhead=False)))
    mesh = M.Mesh(v, f)
    forms = [mesh, (v, f), [v, f], (torch.from_numpy(v), torch.from_numpy(f)), {"vertices": v, "faces": torch.from_numpy(f)}]
    loader = [{"frame_index": torch.tensor([i]), "gt_mesh": g} for i, g in enumerate(forms)]
    res = ev.evaluate_loop(Render(), loader, cfg, device="cpu", quiet=True, evaluator=Keep())
    assert res["count"] == 5 and seen[0] is mesh
    assert seen[1][0] is v and seen[1][1] is f and seen[2][0] is v
    assert torch.equal(seen[3][0], torch.from_numpy(v)) and torch.equal(seen[3][1], torch.from_numpy(f))
    assert seen[4]["vertices"] is v and torch.equal(seen[4]["faces"], torch.from_numpy(f))
