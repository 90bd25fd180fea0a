"""CPU: the host pieces of the field query (gpnerf_query_points) and the coloured mesh -- the PLY export with vertex colours, the
uncoloured export's bytes, the lattice-index mapping against lattice_axis(), the entry point's argument checks and the renderer's
opt-in switch."""
import ctypes as C
import importlib
import io

import numpy as np
import pytest
import torch

import mesh_cases as mc
from golden_cases import load

F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
R = importlib.import_module("gp-nerf_amd.render")
L = importlib.import_module("gp-nerf_amd._lib")

PLY_TYPES = {"double": "<f8", "float": "<f4", "uchar": "u1", "int": "<i4"}


def read_ply_any(data):
    """A binary little-endian PLY reader driven by the header: {element: structured array}, plus the vertex property names."""
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = []
    for line in lines[2:]:
        w = line.split()
        if w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and w[1] == "list":
            assert w[2] == "uchar" and w[4] == "vertex_indices"
            elements[-1][2].append(("n", "u1"))
            elements[-1][2].append(("i", PLY_TYPES[w[3]], (3,)))
        elif w[0] == "property":
            elements[-1][2].append((w[2], PLY_TYPES[w[1]]))
    out, off = {}, 0
    for name, count, fields in elements:
        dt = np.dtype(fields)
        out[name] = np.frombuffer(body, dtype=dt, count=count, offset=off)
        off += count * dt.itemsize
    assert off == len(body)
    return out, [f[0] for f in elements[0][2]]


def todays_ply(vertices, faces):
    """the uncoloured layout as the export wrote it before vertex colours existed"""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {len(v)}\nproperty double x\nproperty double y\nproperty double z\n"
            f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"] = 3
    rec["i"] = f
    return head + v.astype("<f8").tobytes() + rec.tobytes()


def _torus_mesh():
    return mc.marching_cubes_np(mc.torus_field(n=40, R=10.0, r=4.0), 0.02)


def test_coloured_mesh_export_round_trips_through_a_ply_reader(tmp_path):
    v, f = _torus_mesh()
    rng = np.random.default_rng(4)
    col = rng.uniform(0, 1, (len(v), 3)).astype(np.float32)
    col[:6] = [[0, 0, 0], [1, 1, 1], [0.5 / 255, 1.5 / 255, 254.5 / 255], [1e-9, 1 - 1e-7, 0.25], [0.002, 0.998, 0.5], [1, 0, 1]]
    m = M.Mesh(v, f, vertex_colors=col)
    path = tmp_path / "c.ply"
    m.export(str(path))
    data = path.read_bytes()
    el, props = read_ply_any(data)
    assert props == ["x", "y", "z", "red", "green", "blue"]
    vert = el["vertex"]
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), m.vertices)
    want = np.clip(np.rint(np.float32(255) * col), 0, 255).astype(np.uint8)
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), want)
    assert np.array_equal(want[:2], [[0, 0, 0], [255, 255, 255]])
    assert np.all(el["face"]["n"] == 3) and np.array_equal(el["face"]["i"].astype(np.int64), m.faces)
    buf = io.BytesIO()
    m.export(buf)
    assert buf.getvalue() == data
    with pytest.raises(ValueError):
        M.Mesh(v, f, vertex_colors=col[:-1])


def test_uncoloured_mesh_exports_todays_bytes(tmp_path):
    v, f = _torus_mesh()
    m = M.Mesh(v, f)
    assert m.vertex_colors is None
    buf = io.BytesIO()
    m.export(buf)
    assert buf.getvalue() == todays_ply(v, f)
    e = io.BytesIO()
    M.Mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int64)).export(e)
    assert e.getvalue() == todays_ply(np.zeros((0, 3)), np.zeros((0, 3), np.int64))


def lattice_map_np(v, lo, step, pad):
    """the device mapping of gpnerf_query_points' lattice input: float32(lo + (float64(v) - pad) * step), unfused, in float64"""
    return (np.float64(lo) + (np.asarray(v, dtype=np.float32).astype(np.float64) - np.float64(pad)) * np.float64(step)).astype(np.float32)


@pytest.mark.parametrize("name", ["mesh/mesh_body", "mesh/mesh_trained"])
def test_lattice_index_mapping_is_lattice_axis_bit_for_bit(name):
    z, meta = load(name)
    step = np.float64(np.float32(meta["scene_kw"]["voxel"]))       # the scene's float32 voxel size, widened (as the fixture's run)
    box = z["can_bounds"]
    axes = [F.lattice_axis(box[0, a], box[1, a], step) for a in range(3)]
    for a, k in zip(axes, ("axis_x", "axis_y", "axis_z")):
        assert np.array_equal(a.view(np.int32), z[k].view(np.int32)), k
    lo, st, pad = F.lattice_of(axes, [step] * 3)
    assert pad == F.MESH_PAD and np.array_equal(lo, [np.float64(a[0]) for a in axes])
    for a in range(3):
        n = len(axes[a])
        v = (np.arange(n) + pad).astype(np.float32)                  # integer indices of the padded cube, as float32 vertices carry them
        got = lattice_map_np(v, lo[a], st[a], pad)
        assert np.array_equal(got.view(np.int32), axes[a].view(np.int32)), (name, a)


def test_lattice_index_mapping_on_random_boxes():
    rng = np.random.default_rng(12)
    checked = 0
    for _ in range(500):
        lo32 = np.float32(rng.uniform(-2.5, 2.5))
        hi32 = np.float32(lo32 + rng.uniform(0.0, 1.5))
        step = float(rng.choice([0.005, 0.0025, 0.01, 0.0073, np.float64(np.float32(0.005))]))
        ax = F.lattice_axis(lo32, hi32, step)
        lo, st, pad = F.lattice_of([ax] * 3, [step] * 3)
        got = lattice_map_np((np.arange(len(ax)) + pad).astype(np.float32), lo[0], st[0], pad)
        assert np.array_equal(got.view(np.int32), ax.view(np.int32)), (lo32, hi32, step)
        checked += len(ax)
    assert checked > 10000


def _frame(dhw=(8, 8, 8)):
    f = L.GpnerfFrame()
    for l in range(L.LEVELS):
        f.vol[l] = 0x1000
        for a in range(3):
            f.vol_dhw[l][a] = dhw[a]
    f.featmaps, f.feat_h, f.feat_w = 0x1000, 4, 4
    f.imgs, f.img_h, f.img_w = 0x1000, 16, 16
    f.head_blob = f.head_blob_ref = f.occ = 0x1000
    return f


def test_query_points_rejects_bad_arguments_on_the_host():
    lib = L.lib()
    lat = (C.c_double * 7)(0, 0, 0, 0.005, 0.005, 0.005, 10)

    def call(frame, pts=0x1000, n=64, flags=0, lattice=None, raw=0x1000, alpha=None):
        return lib.gpnerf_query_points(C.byref(frame) if frame is not None else None, pts, n, flags, lattice, raw, alpha, None)

    assert call(None) == -1
    assert call(_frame(), n=-1) == -1
    assert call(_frame(), pts=None) == -1
    assert call(_frame(), raw=None) == -1
    assert call(_frame(), raw=None, alpha=0x1000) == -1
    assert call(_frame(), flags=L.FLAG_SPLIT_F16) == -1                     # only NEG_RAY, OCC_CULL and DENSITY_ONLY
    assert call(_frame(), flags=L.FLAG_EARLY_TERM | L.FLAG_NEG_RAY) == -1
    assert call(_frame(), lattice=lat, raw=None) == -1
    for field in ("head_blob_ref", "featmaps", "imgs"):
        f = _frame()
        setattr(f, field, None)
        assert call(f) == -1, field
    f = _frame()
    f.img_h = 0
    assert call(f) == -1
    f = _frame()
    f.vol[2] = None
    assert call(f) == -1
    f = _frame()
    f.occ = None
    assert call(f, flags=L.FLAG_OCC_CULL) == -1                             # the cull reads the occupancy volume
    assert call(_frame(dhw=(4096, 4096, 8))) == -1                          # the frame's own addressing limits (to_framek)
    # n_points == 0 is a no-op (no launch, no device needed), also with empty (NULL) outputs
    assert call(_frame(), n=0, pts=None, raw=None) == 0
    assert call(_frame(), n=0, flags=L.FLAG_OCC_CULL | L.FLAG_NEG_RAY | L.FLAG_DENSITY_ONLY, lattice=lat) == 0


def test_query_points_refuses_cpu_points():
    with pytest.raises(L.GpnerfError, match="no CPU fallback"):
        F.query_points(None, torch.zeros(4, 3))


def test_mesh_colours_are_opt_in(monkeypatch):
    enc, head = torch.nn.Identity(), torch.nn.Identity()
    monkeypatch.delenv("GPNERF_MESH_COLORS", raising=False)
    assert R.Renderer(enc, head).mesh_colors is False
    assert R.Renderer(enc, head, mesh_colors=True).mesh_colors is True
    monkeypatch.setenv("GPNERF_MESH_COLORS", "1")
    assert R.Renderer(enc, head).mesh_colors is True
    assert R.Renderer(enc, head, mesh_colors=False).mesh_colors is False
    monkeypatch.setenv("GPNERF_MESH_COLORS", "0")
    assert R.Renderer(enc, head).mesh_colors is False
