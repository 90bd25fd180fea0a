"""CPU: the adjacency's and the smoothing's entry points refuse bad arguments on the host before anything is launched, the workspace
formula against its header text, the layout's offsets, the wrappers refuse CPU tensors, the Renderer knobs' parsers, and self-checks
of the numpy restatement (tests/smooth_cases.py) the GPU tests compare against: it agrees with mesh_cases.euler_and_closed on the closed
cases, a shuffled face order changes neither its CSR nor a bit of its smoothed vertices, pinned vertices stay, and the smoothing's
property on the binary staircase sphere (the mean normal-to-radial angle more than halves, the volume stays within 1 %) holds for it."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_cases
import simplify_cases as sc
import smooth_cases as sm

P = 0x1000                                                   # a non-null dummy: argument checks never dereference
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpnerf_hip.h")
MAX_FACES = (2 ** 31 - 1) // 3


def _formula(nv, nf):
    """include/gpnerf_hip.h: 256 + 2 a(8 (nv + 1)) + a(nv) + 2 a(16 nv) + 2 a(4 (nv + 1)) + 2 a(4 nv) + a(8 ceil((nv + 1) / 2048)) + 2 a(24 nf)
    + a(3 nf)"""
    a = lambda b: (b + 255) // 256 * 256
    return (256 + 2 * a(8 * (nv + 1)) + a(nv) + 2 * a(16 * nv) + 2 * a(4 * (nv + 1)) + 2 * a(4 * nv) + a(8 * -(-(nv + 1) // 2048))
            + 2 * a(24 * nf) + a(3 * nf))


def test_adjacency_rejects_bad_arguments_on_the_host(pkg):
    lib = pkg._lib.lib()

    def call(faces=P, nf=5, nv=10, ws=P, ws_bytes=1 << 40, stats=P):
        return lib.gpnerf_mesh_adjacency(faces, nf, nv, ws, ws_bytes, stats, None)

    for bad in (dict(faces=None), dict(ws=None), dict(stats=None), dict(nv=-1), dict(nf=-1), dict(nv=1 << 31), dict(nf=MAX_FACES + 1),
                dict(nf=1 << 31), dict(ws_bytes=0), dict(ws_bytes=_formula(10, 5) - 1)):
        assert call(**bad) == -1, bad


def test_smooth_rejects_bad_arguments_on_the_host(pkg):
    lib = pkg._lib.lib()

    def call(vertices=P, nv=10, ws=P, ws_bytes=1 << 40, iterations=10, lam=0.5, mu=-0.53, flags=1, out=P):
        return lib.gpnerf_mesh_smooth(vertices, nv, ws, ws_bytes, iterations, lam, mu, flags, out, None)

    nan, inf = float("nan"), float("inf")
    for bad in (dict(vertices=None), dict(out=None), dict(ws=None), dict(nv=-1), dict(nv=1 << 31), dict(ws_bytes=0),
                dict(ws_bytes=_formula(10, 0) - 1), dict(iterations=-1), dict(iterations=10001), dict(lam=0.0), dict(lam=-0.5), dict(lam=1.5),
                dict(lam=nan), dict(lam=inf), dict(mu=0.1), dict(mu=-1.5), dict(mu=nan), dict(mu=-inf), dict(flags=2), dict(flags=3)):
        assert call(**bad) == -1, bad
    # a mesh without vertices has nothing to launch: accepted, like the boundary values of the factors
    assert call(vertices=None, out=None, nv=0) == 0
    assert call(vertices=None, out=None, nv=0, lam=1.0, mu=-1.0, iterations=10000, flags=0) == 0
    assert call(vertices=None, out=None, nv=0, mu=0.0, iterations=0) == 0


def test_the_workspace_formula_and_the_layout(pkg):
    """the formula as the header prints it, host arithmetic only, 0 for what the calls refuse; the three offsets inside the workspace,
    multiples of 256, and their arrays -- start 8 (nv + 1), neighbours 24 nf, vertex_flags nv bytes -- apart from each other"""
    lib = pkg._lib.lib()
    L = pkg._lib
    text = " ".join(open(HEADER).read().split()).replace(" * ", " ")
    assert ("256 + 2 a(8 (nv + 1)) + a(nv) + 2 a(16 nv) + 2 a(4 (nv + 1)) + 2 a(4 nv) + a(8 ceil((nv + 1) / 2048)) + 2 a(24 nf) + a(3 nf)"
            in text), "the header states the formula this test computes"
    ws = lambda nv, nf: int(lib.gpnerf_mesh_adjacency_workspace_bytes(nv, nf))
    for nv, nf in ((0, 0), (5, 0), (3, 1), (1894, 3784), (2047, 1), (2048, 1), (163842, 327680), (100002, 100000), (2 ** 31 - 1, MAX_FACES)):
        assert ws(nv, nf) == _formula(nv, nf), (nv, nf)
        off = (C.c_int64 * 3)(-1, -1, -1)
        assert lib.gpnerf_mesh_adjacency_layout(nv, nf, off) == 0
        spans = sorted([(off[L.ADJACENCY_START], 8 * (nv + 1)), (off[L.ADJACENCY_NEIGHBOURS], 24 * nf), (off[L.ADJACENCY_VERTEX_FLAGS], nv)])
        assert spans[0][0] >= 256, "the header's words come first"
        for (o, n), nxt in zip(spans, [s[0] for s in spans[1:]] + [ws(nv, nf)]):
            assert o % 256 == 0 and o + n <= nxt, (nv, nf, spans)
        # smooth is not told n_faces: what it reads sits where a mesh of no faces has it
        off0 = (C.c_int64 * 3)()
        assert lib.gpnerf_mesh_adjacency_layout(nv, 0, off0) == 0 and list(off0) == list(off)
    for refused in ((-1, 1), (1, -1), (1 << 31, 1), (1, MAX_FACES + 1)):
        assert ws(*refused) == 0 and lib.gpnerf_mesh_adjacency_layout(*refused, (C.c_int64 * 3)()) == -1, refused
    assert lib.gpnerf_mesh_adjacency_layout(3, 1, None) == -1


def test_the_names_mirror_the_header(pkg):
    hdr = open(HEADER).read()
    L = pkg._lib
    for i, n in enumerate(L.TOPOLOGY_STATS):
        assert re.search(rf"#define GPNERF_TOPOLOGY_{n.upper()} {i}\b", hdr), n
    assert f"#define GPNERF_TOPOLOGY_STATS {len(L.TOPOLOGY_STATS)}" in hdr and tuple(L.TOPOLOGY_STATS) == sm.STATS
    for name, value in (("VERTEX_REFERENCED", L.VERTEX_REFERENCED), ("VERTEX_BOUNDARY", L.VERTEX_BOUNDARY), ("ADJACENCY_START", L.ADJACENCY_START),
                        ("ADJACENCY_NEIGHBOURS", L.ADJACENCY_NEIGHBOURS), ("ADJACENCY_VERTEX_FLAGS", L.ADJACENCY_VERTEX_FLAGS)):
        assert re.search(rf"#define GPNERF_{name} {value}\b", hdr), name
    assert re.search(rf"#define GPNERF_SMOOTH_PIN_BOUNDARY {L.SMOOTH_PIN_BOUNDARY}u\b", hdr)
    assert (L.VERTEX_REFERENCED, L.VERTEX_BOUNDARY) == (sm.REFERENCED, sm.BOUNDARY) and L.ADJACENCY_MAX_FACES == MAX_FACES


def test_cpu_tensors_and_bad_arguments_are_refused(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    v, f = sc.one_triangle()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    for call in (lambda: F.mesh_adjacency(tf, 3), lambda: F.mesh_topology(tf, 3), lambda: F.smooth_mesh(tv, tf)):
        with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
            call()
    for call in (lambda: F.mesh_adjacency(f, 3), lambda: F.mesh_topology(f, 3), lambda: F.smooth_mesh(v, f)):
        with pytest.raises(pkg.GpnerfError, match="device tensor"):
            call()


def test_read_mesh_topology(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    for name in ("tetrahedron", "two_flipped", "three_on_an_edge", "triangle_free", "bad_faces"):
        stats = sm.case(name)[3]["stats"]
        for row in (np.array(sm.stats_row(stats)), torch.tensor(sm.stats_row(stats))):
            assert F.read_mesh_topology(row) == sm.read_topology(stats), name
    t = F.read_mesh_topology(sm.stats_row(sm.case("tetrahedron")[3]["stats"]))
    assert (t["closed"], t["oriented"], t["watertight"], t["euler"]) == (True, True, True, 2)
    t = F.read_mesh_topology(sm.stats_row(sm.case("two_flipped")[3]["stats"]))
    assert (t["closed"], t["oriented"], t["watertight"]) == (False, False, False) and t["inconsistent_edges"] == 1
    with pytest.raises(pkg.GpnerfError):
        F.read_mesh_topology([1, 2, 3])


def test_the_knobs_are_parsed(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    for off in (None, False, 0, 0.0, "0", "", "  "):
        assert F.parse_smooth(off) is None, off
    for on, n in ((3, 3), ("10", 10), (" 2 ", 2), (np.int64(4), 4), (5.0, 5), (10000, 10000)):
        assert F.parse_smooth(on) == n and isinstance(F.parse_smooth(on), int), on
    for bad in (-1, "-2", "taubin", "2.5", 2.5, float("nan"), float("inf"), True, (2,), [3], 10001, "10001"):
        with pytest.raises(pkg.GpnerfError):
            F.parse_smooth(bad)


def test_the_renderer_and_the_evaluator_read_the_knobs(pkg):
    R = importlib.import_module("gp-nerf_amd.render")
    E = importlib.import_module("gp-nerf_amd.evaluator")
    params = inspect.signature(R.Renderer.__init__).parameters
    assert params["mesh_smooth"].default is None and params["mesh_topology"].default is None
    assert inspect.signature(E.MeshEvaluator.__init__).parameters["topology"].default is False
    params = inspect.signature(importlib.import_module("gp-nerf_amd.frame").extract_mesh).parameters
    assert params["smooth"].default is None and params["topology"].default is False
    m = {"clean_stats": torch.arange(6), "simplify_stats": torch.arange(10, 18), "topology_stats": torch.arange(20, 30)}
    L = pkg._lib
    assert list(R.Renderer._mesh_stats(m)) == list(L.CUBE_STATS) + list(L.SIMPLIFY_STATS) + list(L.TOPOLOGY_STATS)
    only = R.Renderer._mesh_stats({"topology_stats": torch.arange(20, 30)})
    assert list(only) == list(L.TOPOLOGY_STATS) and only["faces_used"] == 20 and only["max_valence"] == 29 and len(only) == 10
    assert R.Renderer._mesh_stats({}) is None


# ---- the restatement's self-checks

@pytest.mark.parametrize("name,chi", [("mc_sphere", 2), ("mc_torus", 0), ("ico5", 2), ("binary_sphere", 2), ("tetrahedron", 2)])
def test_the_restatement_agrees_with_the_edge_helper_on_closed_meshes(name, chi):
    v, f, _pin, adj, _one, _ten = sm.case(name)
    assert mesh_cases.euler_and_closed(v, f.astype(np.int64)) == (chi, True, True)
    t = sm.read_topology(adj["stats"])
    assert (t["euler"], t["closed"], t["oriented"], t["watertight"]) == (chi, True, True, True)
    assert t["faces_used"] == len(f) and t["faces_dropped"] == 0 and t["vertices_referenced"] == len(v) and t["boundary_vertices"] == 0
    assert 2 * t["edges"] == 3 * len(f) == int(adj["start"][-1]) == len(adj["neighbours"])
    und = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    assert t["edges"] == len(und)
    assert np.all(adj["vertex_flags"] == sm.REFERENCED)


def test_the_small_cases_come_out_as_the_definition_says():
    row = lambda name: sm.case(name)[3]["stats"]
    assert sm.stats_row(row("empty")) == [0] * 10 and sm.case("empty")[3]["start"].tolist() == [0]
    assert sm.stats_row(row("no_faces")) == [0] * 10 and sm.case("no_faces")[3]["start"].tolist() == [0] * 6
    tri = sm.case("triangle_free")[3]
    assert sm.stats_row(tri["stats"]) == [1, 0, 3, 3, 3, 0, 0, 1, 3, 2]
    assert tri["start"].tolist() == [0, 2, 4, 6] and tri["neighbours"].tolist() == [1, 2, 0, 2, 0, 1] and tri["vertex_flags"].tolist() == [3, 3, 3]
    good, flip = sm.case("two_consistent")[3], sm.case("two_flipped")[3]
    assert sm.stats_row(good["stats"]) == [2, 0, 4, 5, 4, 0, 0, 1, 4, 3] and sm.stats_row(flip["stats"]) == [2, 0, 4, 5, 4, 0, 1, 1, 4, 3]
    assert good["neighbours"].tolist() == flip["neighbours"].tolist() == [1, 2, 3, 0, 2, 0, 1, 3, 0, 2]
    three = sm.case("three_on_an_edge")[3]
    assert sm.stats_row(three["stats"]) == [3, 0, 5, 7, 6, 1, 0, 1, 5, 4] and three["vertex_flags"].tolist() == [3] * 5
    bad = sm.case("bad_faces")[3]
    # faces 0, 1 and 7 are usable; vertex 5 is named by a dropped face only and vertex 6 by none: neither is referenced
    assert sm.stats_row(bad["stats"]) == [3, 5, 5, 7, 5, 0, 0, 1, 5, 4] and bad["vertex_flags"].tolist() == [3, 3, 3, 3, 3, 0, 0]
    assert bad["start"].tolist() == [0, 3, 6, 10, 12, 14, 14, 14]
    # the edge {0, 2} and {1, 2} are shared by two faces in opposite directions: interior; everything else is a border
    assert sm.edges_np(sm.bad_faces()[1], 7)[(0, 2)] == [1, 1] and sm.edges_np(sm.bad_faces()[1], 7)[(1, 2)] == [1, 1]
    fan = sm.case("fan")[3]["stats"]
    assert (fan["max_valence"], fan["edges"], fan["boundary_edges"], fan["euler"]) == (3001, 6001, 3002, 1)


def test_one_pass_written_out_by_hand():
    """the tetrahedron's vertex 0, neighbours 1, 2, 3: x' = float32(x + t (((0.0 + x1) + x2) + x3) / 3 - x)) in float64"""
    v, _f, _pin, adj, one, _ten = sm.case("tetrahedron")
    x = v.astype(np.float64)
    mid = np.empty_like(v)
    for i, nb in enumerate(([1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2])):
        for a in range(3):
            s = 0.0
            for j in nb:
                s = s + x[j, a]
            mid[i, a] = np.float32(x[i, a] + 0.5 * (s / 3.0 - x[i, a]))
    assert np.array_equal(sm.smooth_pass_np(v, adj, 0.5), mid)
    assert np.array_equal(sm.smooth_pass_np(mid, adj, -0.53), one) and not np.array_equal(one, v)
    assert np.array_equal(sm.smooth_np(v, adj, 0), v)


def test_a_shuffled_face_order_changes_nothing_in_the_restatement():
    for name in ("mc_sphere", "fan", "sheet_free"):
        v, f, pin, adj, _one, ten = sm.case(name)
        _v, g = sm.shuffled((v, f))
        assert not np.array_equal(f, g)
        other = sm.adjacency_np(g, len(v))
        assert other["stats"] == adj["stats"] and all(np.array_equal(other[k], adj[k]) for k in ("start", "neighbours", "vertex_flags"))
        assert sm.smooth_np(v, other, sm.ITERATIONS, pin_boundary=pin).tobytes() == ten.tobytes()
    a, s = sm.case("fan"), sm.case("fan_shuffled")
    assert all(np.array_equal(a[3][k], s[3][k]) for k in ("start", "neighbours", "vertex_flags")) and a[5].tobytes() == s[5].tobytes()
    # the long list's one-by-one walk is the rank-by-rank walk
    before = sm.LONG_LIST
    try:
        sm.LONG_LIST = 1 << 20
        assert sm.smooth_np(a[0], a[3], 1, pin_boundary=False).tobytes() == a[4].tobytes()
    finally:
        sm.LONG_LIST = before


def test_pinned_vertices_do_not_move_and_free_ones_do():
    for pinned, free in (("sheet_pinned", "sheet_free"), ("flat_sheet_pinned", "flat_sheet_free"), ("triangle_pinned", "triangle_free"),
                         ("three_on_an_edge", "three_on_an_edge_free")):
        v, _f, _pin, adj, one, ten = sm.case(pinned)
        border = (adj["vertex_flags"] & sm.BOUNDARY) != 0
        assert border.any() and np.array_equal(one[border], v[border]) and np.array_equal(ten[border], v[border])
        moved = sm.case(free)[5]
        assert (moved[border] != v[border]).any(axis=1).all(), free
    v, _f, _pin, adj, _one, ten = sm.case("sheet_pinned")
    inner = (adj["vertex_flags"] & sm.BOUNDARY) == 0
    assert (ten[inner] != v[inner]).any(axis=1).mean() > 0.9
    v, _f, _pin, adj, _one, ten = sm.case("bad_faces")                    # unreferenced vertices never move, pinned or not
    assert np.array_equal(ten[5:], v[5:]) and (ten[:5] != v[:5]).any(axis=1).all()
    v, _f, _pin, _adj, one, ten = sm.case("no_faces")
    assert np.array_equal(one, v) and np.array_equal(ten, v)


def test_values_that_are_not_finite_propagate():
    v, f = sm.tetrahedron()
    v = v.copy()
    v[3, 1] = np.nan
    adj = sm.adjacency_np(f, 4)
    out = sm.smooth_pass_np(v, adj, 0.5)
    assert np.isnan(out[:, 1]).all() and np.isfinite(out[:, [0, 2]]).all()


def test_the_smoothing_property_holds_for_the_restatement():
    """the binary staircase sphere after 10 iterations at the defaults: the mean face-normal-to-radial angle below half the unsmoothed
    mesh's, the enclosed volume within 1 % of it.  Measured with this restatement: 20.65 deg -> 7.17 deg (ratio 0.347), volume + 0.35 %;
    on the already smooth mc_sphere the angle moves by 0.1 deg and the volume by + 0.32 %."""
    v, f, _pin, _adj, _one, ten = sm.case("binary_sphere")
    assert len(v) == 1894
    before, after = sm.normal_angle_deg(v, f, sm.SPHERE_CENTRE), sm.normal_angle_deg(ten, f, sm.SPHERE_CENTRE)
    vol0, vol1 = sm.enclosed_volume(v, f), sm.enclosed_volume(ten, f)
    print(f"binary sphere: angle {before:.2f} -> {after:.2f} deg (ratio {after / before:.3f}), volume {100 * (vol1 / vol0 - 1):+.2f} %")
    assert after < 0.5 * before
    assert abs(vol1 / vol0 - 1.0) < 0.01
    v, f, _pin, _adj, _one, ten = sm.case("mc_sphere")
    print(f"mc_sphere: angle {sm.normal_angle_deg(v, f, sm.SPHERE_CENTRE):.2f} -> {sm.normal_angle_deg(ten, f, sm.SPHERE_CENTRE):.2f} deg, volume "
          f"{100 * (sm.enclosed_volume(ten, f) / sm.enclosed_volume(v, f) - 1):+.2f} %")
    assert abs(sm.enclosed_volume(ten, f) / sm.enclosed_volume(v, f) - 1.0) < 0.01
