"""CPU: the simplification's entry points refuse bad arguments on the host before anything is launched, the workspace formula, the
wrappers refuse CPU tensors, the Renderer knob's parser, and self-checks of the numpy restatement (tests/simplify_cases.py) the GPU
tests compare against."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

import mesh_cases
import simplify_cases as sc

P = 0x1000                                                   # a non-null dummy: argument checks never dereference


def _i3(a, b, c):
    return (C.c_int32 * 3)(a, b, c)


def _f3(a, b, c):
    return (C.c_float * 3)(a, b, c)


def test_count_rejects_bad_arguments_on_the_host(pkg):
    lib = pkg._lib.lib()
    big = 1 << 40

    def call(vertices=P, nv=10, faces=P, nf=5, lo=_f3(0, 0, 0), cell=1.0, cells=_i3(4, 4, 4), ws=P, ws_bytes=big, stats=P):
        return lib.gpnerf_mesh_simplify_count(vertices, nv, faces, nf, lo, cell, cells, ws, ws_bytes, stats, None)

    for bad in (dict(vertices=None), dict(faces=None), dict(lo=None), dict(cells=None), dict(ws=None), dict(stats=None), dict(nv=-1),
                dict(nf=-1), dict(nv=1 << 31), dict(nf=1 << 31), dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")),
                dict(cell=float("inf")), dict(cells=_i3(0, 4, 4)), dict(cells=_i3(4, -1, 4)), dict(cells=_i3(1 << 13, 1 << 13, 2)),
                dict(cells=_i3(1 << 30, 1 << 30, 1 << 30)), dict(lo=_f3(float("nan"), 0, 0))):
        assert call(**bad) == -1, bad
    need = int(lib.gpnerf_mesh_simplify_workspace_bytes(10, 5, _i3(4, 4, 4)))
    assert need > 0 and call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1


def test_emit_rejects_bad_arguments_on_the_host(pkg):
    lib = pkg._lib.lib()
    big = 1 << 40

    def call(vertices=P, nv=10, faces=P, nf=5, ws=P, ws_bytes=big, nov=4, nof=2, ov=P, of=P, vmap=None):
        return lib.gpnerf_mesh_simplify_emit(vertices, nv, faces, nf, ws, ws_bytes, nov, nof, ov, of, vmap, None)

    for bad in (dict(vertices=None), dict(faces=None), dict(ws=None), dict(nv=-1), dict(nf=-1), dict(nv=1 << 31), dict(nf=1 << 31),
                dict(nov=-1), dict(nof=-1), dict(nov=11), dict(nof=6), dict(ov=None), dict(of=None), dict(ws_bytes=0), dict(ws_bytes=255)):
        assert call(**bad) == -1, bad
    need = int(lib.gpnerf_mesh_simplify_workspace_bytes(10, 5, _i3(1, 1, 1)))
    assert call(ws_bytes=need - 1) == -1


def test_the_workspace_formula(pkg):
    """include/gpnerf_hip.h: 256 + 5 a(4 nv) + a(8 (nv + 1)) + a(12 nv) + a(4 nf) + 3 a(12 nf) + a(4 C) + a(8 ceil(max(C, nf, nv + 1) /
    2048)); host arithmetic only; 0 for what the calls refuse"""
    lib = pkg._lib.lib()
    ws = lambda nv, nf, c: int(lib.gpnerf_mesh_simplify_workspace_bytes(nv, nf, _i3(*c) if c is not None else None))
    a = lambda b: (b + 255) // 256 * 256
    for nv, nf, c in ((0, 0, (1, 1, 1)), (3, 1, (2, 2, 1)), (1894, 3784, (13, 13, 13)), (163842, 327680, (130, 70, 45)), (7, 9, (512, 512, 256)),
                      (2 ** 31 - 1, 2 ** 31 - 1, (1 << 26, 1, 1))):
        cc = c[0] * c[1] * c[2]
        want = (256 + 5 * a(4 * nv) + a(8 * (nv + 1)) + a(12 * nv) + a(4 * nf) + 3 * a(12 * nf) + a(4 * cc)
                + a(8 * -(-max(cc, nf, nv + 1) // 2048)))
        assert ws(nv, nf, c) == want, (nv, nf, c)
    for refused in ((-1, 1, (4, 4, 4)), (1, -1, (4, 4, 4)), (1 << 31, 1, (4, 4, 4)), (1, 1 << 31, (4, 4, 4)), (5, 5, (0, 4, 4)), (5, 5, (4, 4, -2)),
                    (5, 5, ((1 << 26) + 1, 1, 1)), (5, 5, (1 << 9, 1 << 9, (1 << 8) + 1)), (5, 5, None)):
        assert ws(*refused) == 0, refused


def test_cpu_tensors_and_bad_shapes_are_refused(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    v, f = sc.one_triangle()
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.simplify_mesh(torch.from_numpy(v), torch.from_numpy(f), 1.0)
    with pytest.raises(pkg.GpnerfError, match="device tensor"):
        F.simplify_mesh(v, f, 1.0)


def test_the_knob_is_parsed(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    for off in (None, False, 0, 0.0, "0", "", "  "):
        assert F.parse_simplify(off) is None, off
    for on, k in ((2, 2.0), (2.5, 2.5), ("3", 3.0), (" 1.5 ", 1.5), (np.float32(4), 4.0), (np.int64(2), 2.0)):
        assert F.parse_simplify(on) == k and isinstance(F.parse_simplify(on), float), on
    for bad in (-1, "-2", "largest", float("nan"), float("inf"), "nan", True, (2,), [3]):
        with pytest.raises(pkg.GpnerfError):
            F.parse_simplify(bad)


def test_the_renderer_reads_the_knob(pkg):
    R = importlib.import_module("gp-nerf_amd.render")
    import inspect
    assert "mesh_simplify" in inspect.signature(R.Renderer.__init__).parameters
    m = {"clean_stats": torch.arange(6), "simplify_stats": torch.arange(10, 18)}
    both = R.Renderer._mesh_stats(m)
    assert list(both) == list(pkg._lib.CUBE_STATS) + list(pkg._lib.SIMPLIFY_STATS) and both["faces_out"] == 11 and both["clusters_dropped"] == 17
    assert R.Renderer._mesh_stats({}) is None
    assert list(R.Renderer._mesh_stats({"simplify_stats": torch.arange(8)})) == list(pkg._lib.SIMPLIFY_STATS)
    assert list(R.Renderer._mesh_stats({"clean_stats": torch.arange(6)})) == list(pkg._lib.CUBE_STATS)


def test_the_stats_names_mirror_the_header(pkg):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpnerf_hip.h")).read()
    L = pkg._lib
    for i, n in enumerate(L.SIMPLIFY_STATS):
        assert re.search(rf"#define GPNERF_SIMPLIFY_{n.upper()} {i}\b", hdr), n
    assert f"#define GPNERF_SIMPLIFY_STATS {len(L.SIMPLIFY_STATS)}" in hdr and tuple(L.SIMPLIFY_STATS) == sc.STATS
    for n in ("HDR_STATUS", "COUNTING", "COUNTED", "EMITTED", "MISMATCH"):
        assert re.search(rf"#define GPNERF_SIMPLIFY_{n} {getattr(L, 'SIMPLIFY_' + n)}\b", hdr), n


def test_simplify_grid_rule(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    lo, cells = F.simplify_grid([3.2, -1.5, 0.0], [10.0, 4.0, 0.0], 2.0)
    assert lo.dtype == np.float32 and lo.tolist() == [2.5, -2.5, -0.5] and cells == [5, 5, 2]
    lo, cells = F.simplify_grid([0.0, 0.0, 0.0], [31.0, 31.0, 31.0], 2.5)
    assert lo.tolist() == [-0.625] * 3 and cells == [14] * 3


# ---- the restatement's self-checks

def _closed_cases():
    for name, mesh, cell, chi in (("sphere", sc.mc_sphere, 2.0, 2), ("sphere", sc.mc_sphere, 2.5, 2), ("torus", sc.mc_torus, 2.5, 0),
                                  ("icosphere", sc.ico5, 2.0, 2)):
        yield pytest.param(mesh, cell, chi, id=f"{name}-{cell}")


@pytest.fixture(scope="module")
def results():
    cache = {}

    def get(mesh, cell):
        key = (mesh.__name__, cell)
        if key not in cache:
            v, f = mesh()
            lo, cells = sc.auto_grid(v, cell)
            cache[key] = (v, f, lo, cells, sc.simplify_np(v, f, lo, cell, cells))
        return cache[key]
    return get


@pytest.mark.parametrize("mesh,cell,chi", _closed_cases())
def test_closed_surfaces_stay_closed(results, mesh, cell, chi):
    """(b): closed, consistently oriented, the input's Euler characteristic; and (a), the sqrt(3) cell bound"""
    v, f, lo, cells, r = results(mesh, cell)
    assert mesh_cases.euler_and_closed(v, f.astype(np.int64)) == (chi, True, True)       # the input is what it is said to be
    s = r["stats"]
    assert len(r["vertices"]) == s["vertices_out"] and len(r["faces"]) == s["faces_out"]
    assert len(f) == s["faces_out"] + s["faces_invalid"] + s["faces_collapsed"] + s["faces_cancelled"] + s["faces_duplicate"]
    assert mesh_cases.euler_and_closed(r["vertices"], r["faces"].astype(np.int64)) == (chi, True, True), s
    assert s["faces_out"] < len(f) / 2 and s["faces_invalid"] == 0
    assert sc.distance_bound_ok(v, f, r, cell, lo, cells) < math.sqrt(3.0)


def test_the_counts_of_the_closed_cases(results):
    """vertices and faces out as an independent prototype of the definition gave them (np.linalg.solve, plain ascending sums)"""
    for mesh, cell, nv, nf, cancelled, dropped in ((sc.mc_sphere, 2.0, 375, 746, 0, None), (sc.mc_sphere, 2.5, 253, 502, 2, 1),
                                                   (sc.mc_torus, 2.5, 500, 1000, 4, 2), (sc.ico5, 2.0, 106, 208, 6, None)):
        s = results(mesh, cell)[4]["stats"]
        assert (s["vertices_out"], s["faces_out"], s["faces_cancelled"]) == (nv, nf, cancelled), (mesh.__name__, cell, s)
        if dropped is not None:
            assert s["clusters_dropped"] == dropped
    assert len(sc.mc_sphere()[1]) == 3784 and len(sc.mc_torus()[1]) == 7416


def test_the_bound_holds_on_the_small_cases():
    """(a) on the hand-made cases"""
    for (v, f), lo, cell, cells in ((sc.one_triangle(), (0, 0, 0), 1.0, (2, 2, 1)), (sc.one_triangle(), (0, 0, 0), 2.0, (1, 1, 1)),
                                    (sc.coincident((1, 1)), (0, 0, 0), 1.0, (2, 2, 1)), (sc.coincident((1, -1)), (0, 0, 0), 1.0, (2, 2, 1)),
                                    (sc.coincident((1, -1, 1)), (0, 0, 0), 1.0, (2, 2, 1)), (sc.bad_faces(), (0, 0, 0), 1.0, (4, 4, 4)),
                                    (sc.flat_sheet(), (0, 0, 0), 1.0, (9, 9, 3)), (sc.fan(300), (0, 0, 0), 1.0, (5, 5, 5))):
        r = sc.simplify_np(v, f, lo, cell, cells)
        sc.distance_bound_ok(v, f, r, cell, lo, cells)
        s = r["stats"]
        assert len(f) == s["faces_out"] + s["faces_invalid"] + s["faces_collapsed"] + s["faces_cancelled"] + s["faces_duplicate"]


def test_the_small_cases_come_out_as_the_definition_says():
    r = sc.simplify_np(*sc.one_triangle(), (0, 0, 0), 1.0, (2, 2, 1))
    assert sc.stats_row(r["stats"]) == [3, 1, 0, 0, 0, 0, r["stats"]["clusters_clamped"], 0] and r["faces"].tolist() == [[0, 2, 1]]
    r = sc.simplify_np(*sc.one_triangle(), (0, 0, 0), 2.0, (1, 1, 1))
    assert sc.stats_row(r["stats"])[:6] == [0, 0, 0, 1, 0, 0] and r["stats"]["clusters_dropped"] == 1 and r["vertex_map"].tolist() == [-1] * 3
    for order in ((1, 1), (-1, -1)):
        r = sc.simplify_np(*sc.coincident(order), (0, 0, 0), 1.0, (2, 2, 1))
        assert sc.stats_row(r["stats"])[:6] == [3, 1, 0, 0, 0, 1]
        assert r["faces"].tolist() == ([[0, 2, 1]] if order[0] > 0 else [[0, 1, 2]])          # the lower index, whichever it is
    r = sc.simplify_np(*sc.coincident((1, -1)), (0, 0, 0), 1.0, (2, 2, 1))
    assert sc.stats_row(r["stats"]) == [0, 0, 0, 0, 2, 0, r["stats"]["clusters_clamped"], 3]
    r = sc.simplify_np(*sc.coincident((1, -1, 1)), (0, 0, 0), 1.0, (2, 2, 1))
    assert sc.stats_row(r["stats"])[:6] == [3, 1, 0, 0, 2, 0] and r["faces"].tolist() == [[0, 2, 1]]
    r = sc.simplify_np(*sc.coincident((-1, 1, -1)), (0, 0, 0), 1.0, (2, 2, 1))
    assert sc.stats_row(r["stats"])[:6] == [3, 1, 0, 0, 2, 0] and r["faces"].tolist() == [[0, 1, 2]]
    v, f = sc.bad_faces()
    r = sc.simplify_np(v, f, (0, 0, 0), 1.0, (4, 4, 4))
    assert sc.stats_row(r["stats"])[:6] == [6, 2, 10, 0, 0, 0]
    # the zero-area face survives, and its clusters, which have no quadric, sit at their cells' centres
    assert r["vertices"][r["faces"][1]].tolist() == [[0.5, 2.5, 2.5], [1.5, 2.5, 2.5], [2.5, 2.5, 2.5]]


def test_a_flat_sheet_stays_flat():
    """(c): z = h off the cell planes: every output vertex within (eps / 3)(cell / 2) of the plane plus a float32 ulp of h, and at
    its cell's centre in x and y (the closed form of step 5 for one normal direction; the shift is along z and stays in the box)"""
    h, cell, n = 1.3, 1.0, 9
    v, f = sc.flat_sheet(n, h, cell)
    r = sc.simplify_np(v, f, (0, 0, 0), cell, (n, n, 3))
    out = r["vertices"].astype(np.float64)
    assert len(out) == n * n and r["stats"]["clusters_clamped"] == 0 and r["stats"]["faces_out"] > 0
    assert np.abs(out[:, 2] - np.float32(h)).max() <= (sc.EPS / 3.0) * (cell / 2.0) + 2.0 ** -23 * h
    assert np.abs(out[:, 2] - np.float32(h)).max() > 0.0                                  # (the regulariser does pull)
    centres = (np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2) + 0.5) * cell
    assert np.array_equal(out[:, :2], centres)
