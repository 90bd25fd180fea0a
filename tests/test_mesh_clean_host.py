"""CPU: the host side of the mesh finishing (gpnerf_cube_clean, gpnerf_mesh_normals) -- the numpy / scipy restatement on the reference's
own cubes (the figures that motivated the feature), the PLY export with normals, the renderer's switches and the entry points'
argument checks."""
import ctypes as C
import importlib
import io

import numpy as np
import pytest
import torch

import mesh_cases as mc
import mesh_clean_cases as cc
from golden_cases import load
from test_field_host import read_ply_any, todays_ply

F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
R = importlib.import_module("gp-nerf_amd.render")
L = importlib.import_module("gp-nerf_amd._lib")
ISO = M.ISO_REFERENCE

# fixture -> (solid components, sizes of the biggest four, surfaces of the raw mesh, cavities after keeping the biggest, their points,
#             triangles of the cleaned mesh)
TABLE = {"mesh/mesh_body": (14, [133654, 313, 85, 9], 54, 39, 201, 76840),
         "mesh/mesh_trained": (37, [50486, 15135, 8751, 8631], 70, 20, 34, 57260)}


@pytest.fixture(scope="module", params=sorted(TABLE))
def golden(request):
    cube = np.ascontiguousarray(load(request.param)[0]["cube"], dtype=np.float32)
    return request.param, cube, mc.marching_cubes_np(cube, ISO)


def test_the_restatement_gives_the_reference_cubes_figures(golden):
    name, cube, (v, f) = golden
    n_comp, biggest, n_surf, n_cav, cav_points, _ = TABLE[name]
    out, labels, stats = cc.clean_np(cube, ISO, cc.KEEP | cc.FILL, 0)
    _, sizes = cc.components(~(cube < np.float32(ISO)), cc.S18)
    assert len(sizes) == n_comp == stats[0]
    assert sorted(sizes.values(), reverse=True)[:4] == biggest
    assert stats[2] == 1 and stats[3] == biggest[0] and stats[1] == sum(sizes.values())
    assert (stats[4], stats[5]) == (n_cav, cav_points)
    assert cc.surfaces(f, len(v)) == n_surf
    # the two connectivities are the case tables': surfaces = solid components (18) + outside components (6) - 1
    _, outside = cc.components(cube < np.float32(ISO), cc.S6)
    assert n_surf == n_comp + len(outside) - 1
    # labels are the lowest linear index of their component
    flat = labels.reshape(-1)
    roots = np.unique(flat[flat >= 0])
    assert np.array_equal(flat[roots], roots) and np.all(flat[flat >= 0] <= np.nonzero(flat >= 0)[0])


def test_largest_plus_fill_leaves_one_surface_of_the_unfiltered_meshs_triangles(golden):
    name, cube, (v, f) = golden
    out, _, _ = cc.clean_np(cube, ISO, cc.KEEP | cc.FILL, 0)
    cv, cf = mc.marching_cubes_np(out, ISO)
    assert len(cf) == TABLE[name][5]
    assert cc.surfaces(cf, len(cv)) == 1
    assert cc.is_subset(cc.triangle_set(cv, cf), cc.triangle_set(v, f)), "a cleaned triangle is not one of the unfiltered mesh's, bit for bit"
    changed = out.view(np.uint32) != cube.view(np.uint32)
    assert np.all(np.isin(out[changed], [0.0, 1.0]))


def test_the_synthetic_cubes_are_what_their_docstrings_say():
    s = cc.snakes_cube()
    _, sizes = cc.components(s >= 0.5, cc.S18)
    assert len(sizes) == 2 and len(set(sizes.values())) == 1 and min(sizes.values()) > 6000
    d, n = cc.diagonal_pairs_cube()
    assert len(cc.components(d >= 0.5, cc.S18)[1]) == n == 16 and int((d >= 0.5).sum()) == 24
    assert list(cc.clean_np(cc.shell_cube(), 0.5, cc.FILL)[2][4:]) == [1, 7 * 12 * 40]
    assert list(cc.clean_np(cc.shell_cube(tunnel=True), 0.5, cc.FILL)[2][4:]) == [0, 0]
    assert list(cc.clean_np(cc.shell_cube(diagonal_leak=True), 0.5, cc.FILL)[2][4:]) == [2, 7 * 12 * 40 + 2]
    fb = cc.floater_bubble_cube()
    assert list(cc.clean_np(fb, 0.5, cc.FILL)[2][4:]) == [1, 6 * 5 * 30]                    # the bubble is a cavity while its floater stands
    assert list(cc.clean_np(fb, 0.5, cc.KEEP | cc.FILL)[2][2:]) == [1, 14 * 11 * 68, 0, 0]   # ... and open once the floater is gone
    n = cc.noise_cube()
    assert cc.clean_np(n, 0.02, cc.KEEP | cc.FILL, 0)[2][4] > 500
    _, sizes = cc.components(~(n < np.float32(cc.NOISE_TIE_ISO)), cc.S18)
    assert len(sizes) > 2000 and sum(1 for v in sizes.values() if v == max(sizes.values())) > 1, "the tie rule decides 'largest'"


def test_mesh_export_with_normals_round_trips(tmp_path):
    v, f = mc.marching_cubes_np(mc.torus_field(n=40, R=10.0, r=4.0), 0.02)
    nrm, _ = cc.normals_np(mc.torus_field(n=40, R=10.0, r=4.0), v)
    col = np.random.default_rng(3).uniform(0, 1, (len(v), 3)).astype(np.float32)
    m = M.Mesh(v, f, vertex_normals=nrm)
    assert m.vertex_normals.dtype == np.float32 and m.vertex_colors is None
    buf = io.BytesIO()
    m.export(buf)
    data = buf.getvalue()
    head = data.split(b"end_header\n")[0].decode("ascii")
    assert "property double z\nproperty float nx\nproperty float ny\nproperty float nz\nelement face" in head
    el, props = read_ply_any(data)
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    vert = el["vertex"]
    assert vert.dtype.itemsize == 24 + 12 and len(data) == len(head) + len("end_header\n") + 36 * len(v) + 13 * len(f)
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), m.vertices)
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1).view(np.uint32), nrm.view(np.uint32))
    assert np.array_equal(el["face"]["i"].astype(np.int64), m.faces)
    path = tmp_path / "n.ply"
    m.export(str(path))
    assert path.read_bytes() == data
    # colours and normals together: x y z nx ny nz red green blue
    both = io.BytesIO()
    M.Mesh(v, f, vertex_colors=col, vertex_normals=nrm).export(both)
    el, props = read_ply_any(both.getvalue())
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and el["vertex"].dtype.itemsize == 39
    assert np.array_equal(np.stack([el["vertex"][k] for k in ("nx", "ny", "nz")], 1), nrm)
    assert np.array_equal(np.stack([el["vertex"][k] for k in ("red", "green", "blue")], 1), M.colour_bytes(col))
    assert np.array_equal(np.stack([el["vertex"][k] for k in ("x", "y", "z")], 1), m.vertices)
    with pytest.raises(ValueError):
        M.Mesh(v, f, vertex_normals=nrm[:-1])
    # without normals: today's bytes
    plain = io.BytesIO()
    M.Mesh(v, f).export(plain)
    assert M.Mesh(v, f).vertex_normals is None and plain.getvalue() == todays_ply(v, f)


def test_mesh_clean_and_normals_are_opt_in(monkeypatch):
    enc, head = torch.nn.Identity(), torch.nn.Identity()
    monkeypatch.delenv("GPNERF_MESH_CLEAN", raising=False)
    monkeypatch.delenv("GPNERF_MESH_NORMALS", raising=False)
    r = R.Renderer(enc, head)
    assert r.mesh_clean is None and r.mesh_normals is False
    assert R.Renderer(enc, head, mesh_clean="largest").mesh_clean == "largest"
    assert R.Renderer(enc, head, mesh_clean=500).mesh_clean == 500
    assert R.Renderer(enc, head, mesh_clean=0).mesh_clean is None
    assert R.Renderer(enc, head, mesh_normals=True).mesh_normals is True
    monkeypatch.setenv("GPNERF_MESH_CLEAN", "largest")
    monkeypatch.setenv("GPNERF_MESH_NORMALS", "1")
    r = R.Renderer(enc, head)
    assert r.mesh_clean == "largest" and r.mesh_normals is True
    assert R.Renderer(enc, head, mesh_clean=False, mesh_normals=False).mesh_clean is None
    assert R.Renderer(enc, head, mesh_clean=False, mesh_normals=False).mesh_normals is False
    monkeypatch.setenv("GPNERF_MESH_CLEAN", "64")
    assert R.Renderer(enc, head).mesh_clean == 64
    monkeypatch.setenv("GPNERF_MESH_CLEAN", "0")
    monkeypatch.setenv("GPNERF_MESH_NORMALS", "0")
    r = R.Renderer(enc, head)
    assert r.mesh_clean is None and r.mesh_normals is False
    for bad in ("biggest", "-3", "1.5"):
        monkeypatch.setenv("GPNERF_MESH_CLEAN", bad)
        with pytest.raises(L.GpnerfError):
            R.Renderer(enc, head)
    with pytest.raises(L.GpnerfError):
        R.Renderer(enc, head, mesh_clean=-1)
    assert F.parse_keep(None) == (0, 0) and F.parse_keep("largest") == (L.CUBE_KEEP, 0) and F.parse_keep(64) == (L.CUBE_KEEP, 64)
    for bad in ("all", 0, -2, 1.5, True):
        with pytest.raises(L.GpnerfError):
            F.parse_keep(bad)


def test_cube_clean_rejects_bad_arguments_on_the_host():
    """GPNERF_E_ARG before any device call: dummy non-null pointers, no GPU needed"""
    lib = L.lib()
    dims = lambda *d: (C.c_int32 * 3)(*d)
    ok = dims(8, 8, 8)
    need = int(lib.gpnerf_cube_clean_workspace_bytes(ok))
    assert need >= 8 * 512 and need < 8 * 512 + 4096
    assert int(lib.gpnerf_cube_clean_workspace_bytes(dims(106, 125, 112))) // (106 * 125 * 112) == 8
    for bad in (dims(1, 8, 8), dims(8, 0, 8), dims(8, 8, -1), dims(1 << 10, 1 << 10, 1 << 9)):
        assert lib.gpnerf_cube_clean_workspace_bytes(bad) == 0
    assert lib.gpnerf_cube_clean_workspace_bytes(None) == 0
    assert lib.gpnerf_cube_clean_workspace_bytes(dims(1 << 10, 1 << 10, 1 << 8)) > 0

    def call(cube=0x100000, d=ok, iso=0.02, flags=L.CUBE_KEEP | L.CUBE_FILL, min_points=0, ws=0x200000, ws_bytes=need, out=0x300000,
             labels=None, stats=0x400000):
        return lib.gpnerf_cube_clean(cube, d, iso, flags, min_points, ws, ws_bytes, out, labels, stats, None)

    assert call(cube=None) == -1 and call(ws=None) == -1 and call(out=None) == -1 and call(stats=None) == -1 and call(d=None) == -1
    assert call(d=dims(1, 8, 8)) == -1 and call(d=dims(1 << 10, 1 << 10, 1 << 9)) == -1
    assert call(out=0x100000) == -1, "out_cube == cube"
    assert call(out=0x100000 + 4 * 511) == -1 and call(cube=0x300000 + 4 * 511) == -1, "partly overlapping cubes"
    assert call(flags=4) == -1 and call(flags=L.CUBE_KEEP | 8) == -1 and call(flags=1 << 31) == -1
    assert call(min_points=-1) == -1
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1
    assert call(iso=float("nan")) == -1
    assert L.CUBE_KEEP == 1 and L.CUBE_FILL == 2 and tuple(L.CUBE_STATS) == cc.STATS
    hdr = open(importlib.import_module("test_abi").HEADER).read()
    assert "#define GPNERF_CUBE_KEEP 1u" in hdr and "#define GPNERF_CUBE_FILL 2u" in hdr


def test_mesh_normals_rejects_bad_arguments_on_the_host():
    lib = L.lib()
    ok = (C.c_int32 * 3)(8, 8, 8)
    call = lambda cube=0x100000, d=ok, v=0x200000, n=4, inv=None, out=0x300000: lib.gpnerf_mesh_normals(cube, d, v, n, inv, out, None)
    assert call(cube=None) == -1 and call(d=None) == -1 and call(d=(C.c_int32 * 3)(8, 1, 8)) == -1
    assert call(v=None) == -1 and call(out=None) == -1 and call(n=-1) == -1
    assert call(n=0) == 0 and call(n=0, v=None, out=None) == 0, "no vertices: a no-op, no launch"


def test_python_wrappers_refuse_cpu_tensors():
    with pytest.raises(L.GpnerfError, match="no CPU fallback"):
        F.cube_clean(torch.zeros(4, 4, 4))
    with pytest.raises(L.GpnerfError, match="no CPU fallback"):
        F.mesh_normals(torch.zeros(4, 4, 4), torch.zeros(3, 3))
