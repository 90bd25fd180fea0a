"""GPU: mesh evaluation on the device (csrc/gpnerf_meshdist.hip) -- the exact point-to-mesh distance in its grid and brute-force forms
(bit-equal to each other, within the float32 bound of the float64 restatement), the grid's build, overflow and bad input, surface
sampling, the stats slot, mesh_metrics and MeshEvaluator end to end, graph capture.

Bounds (tests/mesh_metric_cases.py; none of them taken from what the kernels give): a distance is held to 4 x the largest difference
between THE DISTANCE run in numpy float32 and in float64 on the same inputs, at least 2^-22 max(1, max |coordinate|); the face the
kernel names must be within that bound of the float64 minimum, measured in float64."""
import functools
import importlib
import math
import os
import types

import numpy as np
import pytest
import torch

import mesh_metric_cases as mm
from golden_cases import load

pytestmark = pytest.mark.gpu
F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
L = importlib.import_module("gp-nerf_amd._lib")
ev = importlib.import_module("gp-nerf_amd.evaluator")
DEV = "cuda:0"
INF = float("inf")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def both_forms(points, v, f, max_dist=INF, cell_cap=None, entry_cap=None, normals=None):
    """the grid form and the brute-force form on the same input: asserts dist and face bit-equal, returns the grid form's result as
    numpy arrays and the grid"""
    tv, tf, tp = dev(v), dev(f), dev(points)
    tn = dev(normals) if normals is not None else None
    grid = F.build_mesh_grid(tv, tf, cell_cap, entry_cap)
    g = F.point_mesh_distance(tp, grid=grid, max_dist=max_dist, query_normals=tn, want_closest=True)
    b = F.point_mesh_distance(tp, tv, tf, max_dist=max_dist, query_normals=tn, want_closest=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(g["dist"]), bits(b["dist"])), "dist differs between the grid and the brute-force form"
    assert torch.equal(g["face"], b["face"]), "face differs between the grid and the brute-force form"
    assert torch.equal(bits(g["closest"]), bits(b["closest"]))
    if tn is not None:
        assert torch.equal(bits(g["cosine"]), bits(b["cosine"]))
    return {k: t.cpu().numpy() for k, t in g.items()}, grid


def assert_matches_restatement(what, points, v, f, got, max_dist=INF):
    bound, err, m64, f64, d64 = mm.bound_for(points, v, f)
    dist, face = got["dist"].astype(np.float64), got["face"]
    inside = m64 <= max_dist
    assert np.isfinite(dist[inside]).all() and (face[inside] >= 0).all(), what
    worst = float(np.abs(dist[inside] - m64[inside]).max()) if inside.any() else 0.0
    idx = np.nonzero(inside)[0]
    face_gap = float((d64[idx, face[idx]] - m64[idx]).max()) if inside.any() else 0.0
    print(f"{what}: float32-vs-float64 error {err:.3e} bound {bound:.3e} | dist error {worst:.3e} ratio {worst / bound:.3f} | "
          f"face gap {face_gap:.3e} ratio {face_gap / bound:.3f} | same face as float64 argmin {np.mean(face[idx] == f64[idx]):.3f}")
    assert worst <= bound, what
    assert face_gap <= bound, what
    beyond = m64 > max_dist + bound                            # (within the bound of max_dist either answer is right)
    assert np.isposinf(dist[beyond]).all() and (face[beyond] == -1).all(), what
    undecided = ~inside & ~beyond
    assert (np.isposinf(dist[undecided]) | (np.abs(dist[undecided] - m64[undecided]) <= bound)).all(), what
    hit = np.isfinite(dist)
    if hit.any():                                            # the closest point: at the distance from the query, and on the named face
        p = np.asarray(points, np.float32).astype(np.float64)[hit]
        cp = got["closest"][hit].astype(np.float64)
        assert np.abs(np.linalg.norm(cp - p, axis=1) - dist[hit]).max() <= bound + mm.floor_bound(points, cp), what
        assert mm.distance_to_face(got["closest"][hit], v, f, face[hit]).max() <= bound + mm.floor_bound(points, cp), what
    return bound


# ---- 1. region coverage

@pytest.mark.parametrize("count", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("mesh", ["one_triangle", "two_triangles"])
def test_every_region_of_a_triangle(mesh, count):
    v, f = getattr(mm, mesh)()
    q = mm.region_queries(v, f, count)
    got, _ = both_forms(q, v, f)
    assert_matches_restatement(f"{mesh}[{count}]", q, v, f, got)
    zero = mm.nearest(q, v, f)[0] == 0.0                      # on a vertex, on an edge, in the plane: exactly 0
    assert (got["dist"][zero] == 0.0).all()
    if count == 1000:
        assert zero.sum() >= 7


# ---- 2. degenerate faces

def test_degenerate_faces_are_segments_and_points():
    v, f = mm.degenerate_mix()
    q = mm.degenerate_queries()
    got, grid = both_forms(q, v, f)
    assert not np.isnan(got["dist"]).any() and not np.isnan(got["closest"]).any()
    assert_matches_restatement("degenerate_mix", q, v, f, got)
    assert got["dist"][0] == 0.25 and got["face"][0] == 20       # beside the collinear face: the distance to its segment
    assert got["dist"][2] == 0.5 and got["face"][2] == 20        # beyond its end
    assert got["dist"][4] == 0.0 and got["face"][4] == 20
    assert got["dist"][5] == 0.25 and got["face"][5] == 21       # the face of three equal vertices: the distance to the point
    assert got["dist"][7] == 0.0 and got["face"][7] == 21
    assert (got["face"][8:11] == 3).all() and 22 not in got["face"]          # the duplicated face: its lower index
    h = grid.header()
    assert h["status"] == L.GRID_OK and h["skipped"] == 0 and h["valid"] == 23


# ---- 3. the tie rule

def test_ties_go_to_the_lowest_face_index():
    v, f = mm.tie_cube()
    q = mm.tie_queries()
    d32 = mm.all_distances(q, v, f, np.float32)
    ties = d32 == d32.min(axis=1, keepdims=True)
    assert (ties.sum(axis=1) >= 2).all(), "the restatement's float32 distances are not bit-equal: the case does not test the rule"
    for cell_cap in (None, 1, 512):
        got, _ = both_forms(q, v, f, cell_cap=cell_cap)
        assert got["dist"].tobytes() == d32.min(axis=1).tobytes()              # unfused float32, operation for operation
        assert (got["face"] == ties.argmax(axis=1)).all()
        assert (got["face"] < 2).all() and (ties[:, 10:].any(axis=1)).all()      # +x (faces 0, 1) wins over +y (faces 10, 11)


# ---- 4. icospheres

@pytest.mark.parametrize("level", [2, 3])
def test_icosphere_against_a_concentric_sphere(level):
    v, f = mm.icosphere(level)
    for radius in (1.25, 0.75):
        q = mm.sphere_points(700, radius, seed=level)
        got, _ = both_forms(q, v, f)
        bound = assert_matches_restatement(f"icosphere{level} r={radius}", q, v, f, got)
        # the mean is the radius gap, less (outside) or plus (inside) the sag of the flat faces under the unit sphere -- the sag taken
        # from the restatement: the distance of the unit sphere's own points to the mesh
        unit = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
        sag = mm.nearest(mm.f32(unit), v, f)[0]
        assert 0 < sag.max() < (0.04 if level == 2 else 0.01)
        gap = abs(radius - 1.0)
        mean = float(got["dist"].astype(np.float64).mean())
        lo, hi = (gap, gap + sag.max()) if radius > 1 else (gap - sag.max(), gap)
        assert lo - bound <= mean <= hi + bound, (mean, lo, hi)


# ---- 5. grid stress

def cells_of(grid):
    h = grid.header()
    return h["cells"], h


def test_a_flat_mesh_has_one_cell_across_and_a_cell_size():
    v, f = mm.plane_mesh()
    q = mm.box_queries(v, 500)
    got, grid = both_forms(q, v, f)
    assert_matches_restatement("plane", q, v, f, got)
    cells, h = cells_of(grid)
    assert cells[2] == 1 and h["size"][2] == 1.0 and cells[0] > 1 and cells[1] > 1 and h["n_cells"] == cells[0] * cells[1] <= h["cell_cap"]
    assert abs(cells[0] * h["size"][0] - float(v[:, 0].max() - v[:, 0].min())) < 1e-5
    ratio = h["size"][0] / h["size"][1]
    assert 0.6 < ratio < 1.6                                 # as close to square as whole cell counts allow


@pytest.mark.parametrize("cell_cap", [None, 1, 1 << 20])
def test_one_long_face_among_two_thousand_tiny_ones(cell_cap):
    v, f = mm.stress_mesh()
    q = mm.box_queries(v, 300)
    got, grid = both_forms(q, v, f, cell_cap=cell_cap)
    assert_matches_restatement(f"stress cell_cap={cell_cap}", q, v, f, got)
    cells, h = cells_of(grid)
    print(f"stress cell_cap={cell_cap}: cells {cells} entries {h['needed']} of {h['entry_cap']}")
    assert h["status"] == L.GRID_OK and h["n_cells"] == cells[0] * cells[1] * cells[2] <= h["cell_cap"]
    if cell_cap == 1:
        assert cells == [1, 1, 1] and h["needed"] == len(f)   # the grid has degenerated to brute force
    else:
        assert h["needed"] >= h["n_cells"] * 0.9 + len(f) - 1  # the long face alone is in (nearly) every cell
        assert max(cells) <= 1024 and min(cells) >= 0.8 * max(cells)
    # the entries of every cell are in ascending face index
    lay = grid_layout(h["cell_cap"], h["entry_cap"])
    ws = grid.workspace.cpu().numpy()
    start = ws[lay["start"]:lay["start"] + 4 * (h["n_cells"] + 1)].view(np.int32)
    entries = ws[lay["entries"]:lay["entries"] + 4 * h["needed"]].view(np.int32)
    assert start[0] == 0 and start[-1] == h["needed"] and (np.diff(start) >= 0).all()
    rising = np.diff(entries) > 0
    rising[start[1:-1][(start[1:-1] > 0) & (start[1:-1] < h["needed"])] - 1] = True       # (across a cell boundary anything goes)
    assert rising.all()


def grid_layout(cell_cap, entry_cap):
    """the workspace's regions (csrc/gpnerf_meshdist.hip grid_layout): header, partial boxes, cell starts, cursors, then three int32 [entry_cap] lists"""
    a = lambda n: (n + 255) & ~255
    lay, o = {}, 0
    for name, n in (("hdr", 256), ("part", 32 * 1024), ("start", 4 * (cell_cap + 1)), ("cursor", 4 * cell_cap), ("entries", 4 * entry_cap),
                    ("tmp_face", 4 * entry_cap), ("tmp_cell", 4 * entry_cap)):
        lay[name] = o
        o += a(n)
    lay["total"] = o
    return lay


# ---- 6. far and outside queries

@pytest.mark.parametrize("mesh", ["stress", "icosphere"])
def test_queries_far_outside_the_box(mesh):
    v, f = mm.stress_mesh() if mesh == "stress" else mm.icosphere(2)
    q = mm.far_queries(v)
    assert len(q) == 26
    got, _ = both_forms(q, v, f)
    assert_matches_restatement(f"far {mesh}", q, v, f, got)
    m64 = mm.nearest(q, v, f)[0]
    cut = float(np.float32(0.5 * (m64.min() + m64.max())))                     # between the nearest and the farthest true distance
    assert m64.min() < cut < m64.max()
    got, _ = both_forms(q, v, f, max_dist=cut)
    assert_matches_restatement(f"far {mesh} max_dist={cut}", q, v, f, got, max_dist=cut)
    assert np.isposinf(got["dist"]).sum() >= 6 and np.isfinite(got["dist"]).sum() >= 6
    assert np.isnan(got["closest"][np.isposinf(got["dist"])]).all()


# ---- 7. entry overflow

def test_an_overflowing_grid_says_so_and_writes_no_entry(monkeypatch):
    lib = L.lib()
    v, f = mm.stress_mesh()
    tv, tf = dev(v), dev(f)
    first = F.build_mesh_grid(tv, tf)
    needed, cell_cap = first.header()["needed"], first.cell_cap
    cap = needed - 1
    lay = grid_layout(cell_cap, cap)
    assert lay["total"] == int(lib.gpnerf_mesh_grid_workspace_bytes(len(f), cell_cap, cap))
    guard = 4096
    ws = torch.full((lay["total"] + guard,), 0xA5, device=DEV, dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.gpnerf_mesh_grid_build(tv.data_ptr(), len(v), tf.data_ptr(), len(f), cell_cap, cap, ws.data_ptr(), lay["total"], st) == 0
    grid = F.MeshGrid(tv, tf, ws, cell_cap, cap)
    h = grid.header()
    assert h["status"] == L.GRID_OVERFLOW and h["needed"] == needed and h["entry_cap"] == cap
    assert (ws[lay["entries"]:] == 0xA5).all().item(), "an entry list or the guard behind the workspace has been written"
    q = dev(mm.box_queries(v, 100))
    got = F.point_mesh_distance(q, grid=grid, want_closest=True)
    assert torch.isnan(got["dist"]).all().item() and (got["face"] == -1).all().item() and torch.isnan(got["closest"]).all().item()
    again = F.build_mesh_grid(tv, tf, cell_cap, needed)      # the reported count is enough
    assert again.header()["status"] == L.GRID_OK and again.header()["needed"] == needed
    ok = F.point_mesh_distance(q, grid=again)
    brute = F.point_mesh_distance(q, tv, tf)
    assert torch.equal(bits(ok["dist"]), bits(brute["dist"])) and torch.equal(ok["face"], brute["face"])
    # the wrapper's one retry, forced by a tiny default
    monkeypatch.setattr(importlib.import_module(F.build_mesh_grid.__module__), "mesh_grid_caps", lambda n_faces: (cell_cap, 16))
    retried = F.build_mesh_grid(tv, tf)
    assert retried.entry_cap == needed and retried.header()["status"] == L.GRID_OK
    unchecked = F.build_mesh_grid(tv, tf, check=False)
    assert unchecked.entry_cap == 16 and unchecked.header()["status"] == L.GRID_OVERFLOW


# ---- 8. bad input

def test_bad_faces_are_skipped_and_bad_queries_get_nan():
    v, f = mm.icosahedron()
    v = np.concatenate([v, mm.f32([[np.nan, 0, 0], [0, np.inf, 0]])])
    nv = len(v)
    f = np.concatenate([f[:5], [[0, 1, -1]], f[5:12], [[0, nv, 2]], [[3, 12, 4]], f[12:], [[13, 1, 2]], [[2 ** 31 - 1, 0, 1]]]).astype(np.int32)
    assert (~mm.valid_faces(v, f)).sum() == 5
    q = np.concatenate([mm.sphere_points(60, 1.5, seed=8), mm.f32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.5, 0.5, 0.5]])])
    normals = np.tile(mm.f32([[0, 0, 1]]), (len(q), 1))
    got, grid = both_forms(q, v, f, normals=normals)
    h = grid.header()
    assert h["skipped"] == 5 and h["valid"] == 20 and h["status"] == L.GRID_OK
    good = np.isfinite(q).all(axis=1)
    assert np.isnan(got["dist"][~good]).all() and (got["face"][~good] == -1).all()
    assert np.isnan(got["closest"][~good]).all() and np.isnan(got["cosine"][~good]).all()
    sub = {k: a[good] for k, a in got.items()}
    assert_matches_restatement("bad faces", q[good], v, f, sub)
    assert mm.valid_faces(v, f)[sub["face"]].all()
    # the cosine: |n_q . n_f| with the nearest face's float32 unit normal
    tri = v[f[sub["face"]]].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    want = np.abs(n[:, 2]) / np.linalg.norm(n, axis=1)
    assert np.abs(sub["cosine"] - want).max() <= 1e-6       # a handful of float32 roundings of values no larger than 1
    # a mesh with no valid face at all: +inf / -1, in both forms
    none = np.array([[0, 1, -1], [12, 1, 2]], np.int32)
    got, grid = both_forms(q[good], v, none)
    assert np.isposinf(got["dist"]).all() and (got["face"] == -1).all() and grid.header()["valid"] == 0


# ---- 9. sampling

@pytest.mark.parametrize("mesh", ["stress", "icosphere", "with_flat_faces"])
def test_samples_lie_on_their_faces_in_proportion_to_area(mesh):
    v, f = {"stress": mm.stress_mesh, "icosphere": lambda: mm.icosphere(2), "with_flat_faces": mm.degenerate_mix}[mesh]()
    n = 5000
    tv, tf = dev(v), dev(f)
    s = F.sample_surface(tv, tf, n, seed=3)
    pts, face, normal = s["points"].cpu().numpy(), s["face"].cpu().numpy(), s["normal"].cpu().numpy()
    assert s["workspace"][:4].cpu().numpy().view(np.int32)[0] == L.SAMPLE_OK
    area = mm.face_areas(v, f)
    counts = np.bincount(face, minlength=len(f))
    share = n * area / area.sum()
    print(f"sampling {mesh}: largest |count - share| {np.abs(counts - share).max():.6f}")
    assert np.abs(counts - share).max() < 1 + 1e-6
    assert (counts[area == 0] == 0).all() and (np.diff(face) >= 0).all()
    # on the face, by the distance rule: bound = 4 x the largest distance between a sample's float32 point and the same formula in
    # float64 (which lies in the face's plane), at least 2^-22 max(1, max |coordinate|).  The bound is a LENGTH.  A barycentric
    # coordinate is a length over the face's altitude, so it is held to bound / (the face's smallest altitude): the float32 grid of
    # the output alone (6e-8 at coordinates near 1) is 2e-5 of a tiny stress face's 0.003 altitude, so `>= -bound` as a bare
    # number cannot hold there for any code that returns float32 points (measured on the stress mesh: lowest -9.6e-7, bound 6.7e-7)
    bound, err = mm.sampling_bound(v, f, face, 3)
    bary, off = mm.barycentrics(pts, v, f, face)
    tri = v[f[face]].astype(np.float64)
    longest = np.max([np.linalg.norm(tri[:, (k + 1) % 3] - tri[:, k], axis=1) for k in range(3)], axis=0)
    altitude = 2 * area[face] / longest
    print(f"sampling {mesh}: float32-vs-float64 error {err:.3e} bound {bound:.3e} | off-plane {off.max():.3e} ratio {off.max() / bound:.3f} | "
          f"lowest barycentric {bary.min():.3e}, as a length {(bary.min(axis=1) * altitude).min():.3e} "
          f"ratio {(-bary.min(axis=1) * altitude).max() / bound:.4f}")
    assert off.max() <= bound
    assert (bary.min(axis=1) * altitude >= -bound).all() and (np.abs(bary.sum(axis=1) - 1) * altitude <= bound).all()
    n64 = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert np.abs(normal - n64 / np.linalg.norm(n64, axis=1, keepdims=True)).max() < 1e-5
    # the first ten samples, bit for bit, from the restated hash and the header's order of operations
    r1, r2 = mm.sample_randoms(3, np.arange(10))
    want = np.stack([mm.sample_point(v, f[face[i]], r1[i], r2[i]) for i in range(10)])
    assert want.dtype == np.float32 and pts[:10].tobytes() == want.tobytes()
    # the same call again, and under graph replay: the same bits; another seed: other points on the same faces
    s2 = F.sample_surface(tv, tf, n, seed=3)
    assert torch.equal(bits(s2["points"]), bits(s["points"])) and torch.equal(s2["face"], s["face"]) and torch.equal(bits(s2["normal"]), bits(s["normal"]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s3 = F.sample_surface(tv, tf, n, seed=3)
    for _ in range(2):
        s3["points"].fill_(7.0)
        s3["workspace"].fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(s3["points"]), bits(s["points"])) and torch.equal(s3["face"], s["face"])
    other = F.sample_surface(tv, tf, n, seed=4)
    assert torch.equal(other["face"], s["face"]) and not torch.equal(bits(other["points"]), bits(s["points"]))


def test_samples_are_uniform_on_one_triangle_and_nan_without_area():
    v, f = mm.one_triangle()
    s = F.sample_surface(dev(v), dev(f), 4096, seed=0)
    bary, _ = mm.barycentrics(s["points"].cpu().numpy(), v, f, s["face"].cpu().numpy())
    print(f"one triangle: mean barycentrics {bary.mean(axis=0)}")
    assert np.abs(bary.mean(axis=0) - 1 / 3).max() < 0.02    # sigma of a mean of 4096: sqrt(1 / 18 / 4096) = 0.0037
    flat = F.sample_surface(dev(mm.f32([[0, 0, 0], [1, 0, 0], [2, 0, 0]])), dev(f), 100, seed=0)
    assert flat["workspace"][:4].cpu().numpy().view(np.int32)[0] == L.SAMPLE_NO_AREA
    assert torch.isnan(flat["points"]).all().item() and (flat["face"] == -1).all().item()
    assert F.sample_surface(dev(v), dev(f), 0)["points"].shape == (0, 3)
    # a face with a non-finite vertex is invalid here as everywhere: no area, no sample, and the others keep their shares
    v, f = mm.icosahedron()
    v = v.copy()
    v[7] = [np.nan, 0, np.inf]
    s = F.sample_surface(dev(v), dev(f), 600, seed=0)
    face = s["face"].cpu().numpy()
    area = mm.face_areas(v, f)
    assert s["workspace"][:4].cpu().numpy().view(np.int32)[0] == L.SAMPLE_OK and (area == 0).sum() == 5
    assert torch.isfinite(s["points"]).all().item() and (area[face] > 0).all()
    assert np.abs(np.bincount(face, minlength=20) - 600 * area / area.sum()).max() < 1 + 1e-6


# ---- 10. stats

@pytest.mark.parametrize("n", [0, 1, 65, 100003])
def test_stats_slot(n):
    values = mm.stats_values(n)
    th = (0.01, 0.025, 0.04, 0.05)
    slot = F.distance_stats(dev(values), th).cpu().numpy()
    fin, inf, nan, mean, sq, mx, within, nonnan = mm.stats_np(values, th)
    assert [slot[L.DIST_FINITE], slot[L.DIST_INF], slot[L.DIST_NAN]] == [fin, inf, nan] and fin + inf + nan == n
    assert n < 1000 or np.isneginf(values).sum() > 10       # -inf is among them: counted under INF, within no threshold
    if fin:
        assert abs(slot[L.DIST_MEAN] / mean - 1) <= 1e-12 and abs(slot[L.DIST_MEAN_SQ] / sq - 1) <= 1e-12 and slot[L.DIST_MAX] == mx
    else:
        assert np.isnan(slot[[L.DIST_MEAN, L.DIST_MEAN_SQ, L.DIST_MAX]]).all()
    for k in range(4):
        if nonnan:
            assert slot[L.DIST_WITHIN + k] == within[k] / nonnan
        else:
            assert np.isnan(slot[L.DIST_WITHIN + k])
    two = F.distance_stats(dev(values), th[:2]).cpu().numpy()
    assert two[:L.DIST_WITHIN + 2].tobytes() == slot[:L.DIST_WITHIN + 2].tobytes() and np.isnan(two[L.DIST_WITHIN + 2:]).all()


# ---- 11. body size, once

@functools.lru_cache(maxsize=None)
def golden_mesh(name):
    z, _ = load(name)
    verts, faces = F.marching_cubes(dev(np.ascontiguousarray(z["cube"], dtype=np.float32)), float(z["iso"]))
    return verts, faces


def test_body_sized_grid_against_brute_force_and_the_restatement():
    bv, bf = golden_mesh("mesh/mesh_body")
    tv, tf = golden_mesh("mesh/mesh_trained")
    assert bf.shape[0] > 50000
    s = F.sample_surface(tv, tf, 4096, seed=1)
    grid = F.build_mesh_grid(bv, bf)
    g = F.point_mesh_distance(s["points"], grid=grid, query_normals=s["normal"])
    b = F.point_mesh_distance(s["points"], bv, bf, query_normals=s["normal"])
    assert torch.equal(bits(g["dist"]), bits(b["dist"])) and torch.equal(g["face"], b["face"]) and torch.equal(bits(g["cosine"]), bits(b["cosine"]))
    h = grid.header()
    print(f"body: {bf.shape[0]} faces, cells {h['cells']}, entries {h['needed']} of {h['entry_cap']}")
    assert h["status"] == L.GRID_OK and h["skipped"] == 0
    pick = np.linspace(0, 4095, 64).astype(int)
    q, v, f = s["points"].cpu().numpy()[pick], bv.cpu().numpy(), bf.cpu().numpy()
    d64, d32 = mm.nearest_pruned(q, v, f)
    err = float(np.abs(d32 - d64).max())
    bound = max(4 * err, mm.floor_bound(q, v))
    dist, face = g["dist"].cpu().numpy()[pick].astype(np.float64), g["face"].cpu().numpy()[pick]
    gap = mm.distance_to_face(q, v, f, face) - d64
    print(f"body: float32-vs-float64 error {err:.3e} bound {bound:.3e} | dist error {np.abs(dist - d64).max():.3e} "
          f"ratio {np.abs(dist - d64).max() / bound:.3f} | face gap {gap.max():.3e}")
    assert np.abs(dist - d64).max() <= bound and gap.max() <= bound


# ---- 12. end to end

def test_a_mesh_against_itself():
    for name, (v, f) in (("icosphere", mm.icosphere(2)), ("cube", mm.cube_mesh())):
        th = (0.001, 0.01)
        slots = F.mesh_metrics((v, f), M.Mesh(v, f), n_samples=20000, thresholds=th, seed=5, device=DEV)
        assert slots.shape == (4, L.DIST_DOUBLES) and slots.is_cuda
        r = F.read_mesh_metrics(slots, th)
        pts = F.sample_surface(dev(v), dev(f), 20000, seed=5)["points"][:256].cpu().numpy()
        bound = mm.bound_for(pts, v, f)[0]
        print(f"{name} against itself: {r} bound {bound:.3e}")
        assert 0 <= r["accuracy"] <= bound and 0 <= r["completeness"] <= bound and r["chamfer"] <= bound
        assert r["normal_consistency"] >= 1 - 1e-5
        assert all(r[f"fscore@{t:g}"] == 1.0 for t in th)
        assert r["n_pred"] == r["n_gt"] == 20000 and r["nan_pred"] == r["beyond_gt"] == 0


def test_a_cube_against_itself_shifted():
    h, n = 0.25, 3000
    v, f = mm.cube_mesh()
    v2 = mm.f32(v.astype(np.float64) + [h, 0, 0])
    th = (0.1, 0.25, 0.3)
    r = F.read_mesh_metrics(F.mesh_metrics((v, f), (v2, f), n_samples=n, thresholds=th, seed=2, device=DEV), th)
    for key, (mesh, other, seed) in (("accuracy", ((v, f), (v2, f), 2)), ("completeness", ((v2, f), (v, f), 3))):
        s = F.sample_surface(dev(mesh[0]), dev(mesh[1]), n, seed=seed)
        pts, face = s["points"].cpu().numpy(), s["face"].cpu().numpy()
        bound, _, m64, _, _ = mm.bound_for(pts, *other)
        assert abs(r[key] - m64.mean()) <= bound, key
        # the faces normal to x (quads 0: +x, 1: -x).  The one that the shift carries OUT of the other cube has every sample at h
        # exactly; on the one carried INTO it a sample near the rim is nearer to a side face, so h is its upper bound
        outer, inner = (face // 2 == 1, face // 2 == 0) if key == "accuracy" else (face // 2 == 0, face // 2 == 1)
        assert outer.sum() > n / 8 and np.abs(m64[outer] - h).max() <= mm.floor_bound(pts)
        assert inner.sum() > n / 8 and m64[inner].max() <= h + mm.floor_bound(pts) and (np.abs(m64[inner] - h) <= mm.floor_bound(pts)).mean() > 0.4
        assert abs(r[key + "_max"] - m64.max()) <= bound
        frac = [(m64 <= t).mean() for t in th]
        name = "precision" if key == "accuracy" else "recall"
        assert abs(r[f"{name}@0.1"] - frac[0]) <= 2 / n and r[f"{name}@0.3"] == 1.0
    assert r["chamfer"] == 0.5 * (r["accuracy"] + r["completeness"]) and abs(r["accuracy"] - r["completeness"]) < 0.02
    assert 0.5 < r["normal_consistency"] <= 1.0
    # max_dist below the shift: the x faces' samples are beyond it
    cut = F.read_mesh_metrics(F.mesh_metrics((v, f), (v2, f), n_samples=n, thresholds=th, seed=2, max_dist=0.2, device=DEV), th)
    assert cut["beyond_pred"] > n / 5 and cut["n_pred"] + cut["beyond_pred"] == n and cut["accuracy"] < r["accuracy"]


def _frames(tmp_path):
    rng = np.random.default_rng(4)
    axes = [np.linspace(-0.2, 0.2, 9).astype(np.float32), np.linspace(0.0, 0.5, 11).astype(np.float32), np.linspace(-0.1, 0.1, 5).astype(np.float32)]
    out = []
    for i in range(3):
        cube = np.pad(rng.uniform(0, 0.04, (9, 11, 5)).astype(np.float32), 10)
        v, f = mm.cube_mesh(half=1.5 + 0.25 * i, centre=(14, 15, 12))          # index units of the padded cube
        pred = M.Mesh(v, f)
        gt = pred.to_lattice_frame(axes, 10)
        gt = M.Mesh(gt.vertices + [0.0, 0.001 * (i + 1), 0.0], gt.faces)
        out.append(({"cube": cube, "mesh": pred, "axes": axes}, {"frame_index": torch.tensor([i]), "gt_mesh": gt}))
    return out


def test_mesh_evaluator_over_three_frames(tmp_path, capsys):
    frames = _frames(tmp_path)
    e = ev.MeshEvaluator(str(tmp_path / "a"), 0.02, metric_samples=4000, metric_thresholds=(0.0005, 0.005))
    assert not e.has_mesh_metrics
    for output, batch in frames:
        e.evaluate(output, batch)
    assert e.has_mesh_metrics
    s = e.summarize()
    per = s.pop("per_frame")
    assert per["frame_index"] == [0, 1, 2] and all(len(v) == 3 for v in per.values())
    assert set(s) == set(per) - {"frame_index"} and {"accuracy", "completeness", "chamfer", "normal_consistency", "fscore@0.005"} <= set(s)
    assert all(s[k] == float(np.mean(per[k])) for k in s)
    # a box moved by d along y: the four faces along y stay in their planes, the two others are at d
    for i in range(3):
        d = 0.001 * (i + 1)
        assert 0.2 * d < per["accuracy"][i] < 0.5 * d and abs(per["accuracy_max"][i] - d) < 1e-6 and per["fscore@0.005"][i] == 1.0
    table = np.load(tmp_path / "a" / "mesh_metrics.npy")
    assert len(table) == 3 and table["frame_index"].tolist() == [0, 1, 2] and table["chamfer"].tolist() == per["chamfer"]
    assert sorted(os.listdir(tmp_path / "a")) == ["mesh_metrics.npy", "pts"]
    assert e.summarize() == {} and not e.has_mesh_metrics      # reset
    # without gt_mesh: what it did before
    b = ev.MeshEvaluator(str(tmp_path / "b"), 0.02)
    for output, batch in frames:
        b.evaluate(output, {"frame_index": batch["frame_index"]})
    assert b.summarize() == {} and os.listdir(tmp_path / "b") == ["pts"]
    # an output without axes (the points then come from the batch's pts): the mesh is taken as it is, already in the scan's frame
    c = ev.MeshEvaluator(str(tmp_path / "c"), 0.02, metric_samples=2000, metric_entry_cap=4096)
    output, batch = frames[0]
    placed = output["mesh"].to_lattice_frame(output["axes"], 10)
    pts = torch.from_numpy(np.stack(np.meshgrid(*output["axes"], indexing="ij"), axis=-1))[None]
    c.evaluate({"cube": output["cube"], "mesh": placed}, {"frame_index": torch.tensor([9]), "pts": pts, "gt_mesh": batch["gt_mesh"]})
    got = c.summarize()
    assert abs(got["accuracy"] - per["accuracy"][0]) < 1e-4 and abs(got["accuracy_max"] - 0.001) < 1e-6
    # ... and the same mesh handed over in index units WITH axes must not be taken as it is
    d = ev.MeshEvaluator(str(tmp_path / "d"), 0.02, metric_samples=2000)
    d.evaluate({"cube": output["cube"], "mesh": placed, "axes": output["axes"]}, {"frame_index": torch.tensor([9]), "gt_mesh": batch["gt_mesh"]})
    assert d.summarize()["accuracy"] > 0.1


@pytest.mark.parametrize("form", ["mesh", "numpy_pair", "tensor_pair"])
def test_the_loop_returns_the_mesh_metrics(tmp_path, form):
    """gt_mesh in each form the evaluator documents, through evaluate_loop's move to the device: a Mesh and numpy arrays stay on the
    host as they are, tensors are moved; the numbers are the same"""
    frames = _frames(tmp_path)

    def handed(m):
        if form == "mesh":
            return m
        if form == "numpy_pair":
            return (m.vertices, m.faces)
        return (torch.from_numpy(m.vertices), torch.from_numpy(m.faces))

    class Render(torch.nn.Module):
        nerfhead = types.SimpleNamespace(use_rgbhead=False)
        at = 0

        def render(self, batch):
            self.at += 1
            return dict(frames[self.at - 1][0], rtime=0.25)

    cfg = types.SimpleNamespace(test=types.SimpleNamespace(test_seq="s"), head=types.SimpleNamespace(rgb=types.SimpleNamespace(use_rgbhead=False)))
    e = ev.MeshEvaluator(str(tmp_path), 0.02, metric_samples=2000)
    res = ev.evaluate_loop(Render(), [dict(b, gt_mesh=handed(b["gt_mesh"])) for _, b in frames], cfg, device=DEV, quiet=True, evaluator=e)
    assert res["count"] == 3 and res["metrics"] is not None and res["metrics"]["per_frame"]["frame_index"] == [0, 1, 2]
    assert res["metrics"]["chamfer"] > 0 and res["mse"] == []
    assert os.path.exists(tmp_path / "mesh_metrics.npy")
    direct = ev.MeshEvaluator(str(tmp_path / "direct"), 0.02, metric_samples=2000)
    for output, batch in frames:
        direct.evaluate(output, batch)
    assert direct.summarize()["per_frame"]["chamfer"] == res["metrics"]["per_frame"]["chamfer"]


# ---- 13. graph capture

def test_build_distance_and_stats_capture_into_a_graph():
    v, f = mm.stress_mesh()
    tv, tf, q = dev(v), dev(f), dev(mm.box_queries(v, 1000))
    th = (0.01, 0.05)

    def run():
        grid = F.build_mesh_grid(tv, tf, check=False)
        res = F.point_mesh_distance(q, grid=grid, want_closest=True)
        return grid, res, F.distance_stats(res["dist"], th)

    _, eager, eager_slot = run()                             # (also loads the kernels before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        grid, res, slot = run()
    for _ in range(3):
        grid.workspace.fill_(0xA5)                           # the workspace carries nothing from call to call
        res["dist"].fill_(-1.0)
        res["face"].fill_(-7)
        slot.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(res["dist"]), bits(eager["dist"])) and torch.equal(res["face"], eager["face"])
        assert torch.equal(bits(res["closest"]), bits(eager["closest"]))
        assert slot.cpu().numpy().tobytes() == eager_slot.cpu().numpy().tobytes()
    assert grid.header()["status"] == L.GRID_OK
