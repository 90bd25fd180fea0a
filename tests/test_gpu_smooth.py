"""GPU: the mesh adjacency, the topology counts and the Taubin smoothing (gpnerf_meshtopo.hip) against the numpy restatement of
include/gpnerf_hip.h (tests/smooth_cases.py): stats, start, the used part of neighbours and vertex_flags EQUAL, the smoothed vertices
BIT-EQUAL after 1 and after 10 iterations (both sides spell the same float64 adds, one divide and one multiply in the same order); a
shuffled face order changes nothing; two runs and a graph replay identical; the smoothing's property on the binary staircase sphere;
extract_mesh(smooth=, topology=), Renderer(mesh_smooth=, mesh_topology=) and MeshEvaluator(topology=True) end to end.

Measured on an MI355X: 0 of the 117 948 coordinates of the 20 cases (1 and 10 iterations) and 0 of the 120 168 of the golden body mesh after
3 iterations were not bit-equal."""
import functools
import importlib
import os
import sys
import types
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import mesh_cases as mc
import mesh_metric_cases as mm
import simplify_cases as sc
import smooth_cases as sm
from golden_cases import load, scene_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = importlib.import_module("gp-nerf_amd.frame")
R = importlib.import_module("gp-nerf_amd.render")
L = importlib.import_module("gp-nerf_amd._lib")
M = importlib.import_module("gp-nerf_amd.mesh")
ev = importlib.import_module("gp-nerf_amd.evaluator")
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def device_result(name):
    """(stats, start, neighbours in use, vertex_flags, vertices after 1 iteration, after 10, after 0) on the host"""
    v, f, pin, *_ = sm.case(name)
    tv, tf = dev(v), dev(f)
    adj = F.mesh_adjacency(tf, len(v))
    one = F.smooth_mesh(tv, adjacency=adj, iterations=1, pin_boundary=pin)
    ten = F.smooth_mesh(tv, adjacency=adj, iterations=sm.ITERATIONS, lam=sm.LAM, mu=sm.MU, pin_boundary=pin)
    zero = F.smooth_mesh(tv, adjacency=adj, iterations=0, pin_boundary=pin)
    torch.cuda.synchronize()
    start = adj.start.cpu().numpy()
    assert adj.neighbours.shape == (6 * len(f),) and adj.vertex_flags.shape == (len(v),) and adj.stats.shape == (10,)
    return (adj.stats.cpu().numpy(), start, adj.neighbours[:int(start[-1])].cpu().numpy(), adj.vertex_flags.cpu().numpy(), one.cpu().numpy(),
            ten.cpu().numpy(), zero.cpu().numpy())


BITS = {"coordinates": 0, "differing": 0}


@pytest.mark.parametrize("name", list(sm.CASES))
def test_adjacency_and_smoothing_are_the_restatement(name):
    v, f, pin, ref, ref_one, ref_ten = sm.case(name)
    stats, start, nb, flags, one, ten, zero = device_result(name)
    print(name, dict(zip(L.TOPOLOGY_STATS, stats.tolist())))
    assert stats.dtype == np.int64 and stats.tolist() == sm.stats_row(ref["stats"])
    assert start.dtype == np.int64 and np.array_equal(start, ref["start"])
    assert nb.dtype == np.int32 and np.array_equal(nb, ref["neighbours"])
    assert flags.dtype == np.uint8 and np.array_equal(flags, ref["vertex_flags"])
    assert zero.dtype == np.float32 and zero.tobytes() == v.tobytes()
    for what, got, want in (("1 iteration", one, ref_one), (f"{sm.ITERATIONS} iterations", ten, ref_ten)):
        assert got.dtype == np.float32 and got.shape == want.shape
        differing = int((got.view(np.uint32) != want.view(np.uint32)).sum()) if got.size else 0
        BITS["coordinates"] += got.size
        BITS["differing"] += differing
        print(f"{name}, {what}: {differing} of {got.size} coordinates not bit-equal; so far {BITS['differing']} of {BITS['coordinates']}")
        assert got.tobytes() == want.tobytes(), (name, what, differing)


def test_the_cases_reach_their_branches():
    row = lambda name: dict(zip(L.TOPOLOGY_STATS, device_result(name)[0].tolist()))
    assert device_result("empty")[1].tolist() == [0] and device_result("empty")[4].shape == (0, 3)
    assert row("triangle_free")["boundary_edges"] == 3 and row("two_flipped")["inconsistent_edges"] == 1 and row("two_consistent")["inconsistent_edges"] == 0
    assert row("three_on_an_edge")["nonmanifold_edges"] == 1 and row("bad_faces")["faces_dropped"] == 5
    assert device_result("bad_faces")[3].tolist() == [3, 3, 3, 3, 3, 0, 0]
    for name, chi in (("tetrahedron", 2), ("mc_sphere", 2), ("mc_torus", 0), ("ico5", 2), ("binary_sphere", 2)):
        t = F.read_mesh_topology(device_result(name)[0])
        v, f = sm.case(name)[:2]
        assert (t["euler"], t["closed"], t["oriented"], t["watertight"]) == (chi, True, True, True), name
        assert mc.euler_and_closed(v, f.astype(np.int64)) == (chi, True, True)
    assert 3 * len(sc.mc_sphere()[1]) == 11352 > 5 * 2048            # the half-edges cross the scan's blocks
    assert row("fan")["max_valence"] == 3001
    # pinned borders stay, free ones move
    for pinned, free in (("sheet_pinned", "sheet_free"), ("flat_sheet_pinned", "flat_sheet_free"), ("triangle_pinned", "triangle_free")):
        v = sm.case(pinned)[0]
        border = (device_result(pinned)[3] & L.VERTEX_BOUNDARY) != 0
        assert border.any() and np.array_equal(device_result(pinned)[5][border], v[border])
        assert (device_result(free)[5][border] != v[border]).any(axis=1).all()


def test_the_face_order_changes_no_bit():
    a, s = device_result("fan"), device_result("fan_shuffled")
    assert not np.array_equal(sm.case("fan")[1], sm.case("fan_shuffled")[1])
    for k in range(7):
        assert a[k].tobytes() == s[k].tobytes(), k
    v, f = sc.mc_sphere()
    _v, g = sm.shuffled((v, f))
    adj = F.mesh_adjacency(dev(g), len(v))
    ten = F.smooth_mesh(dev(v), adjacency=adj)
    ref = device_result("mc_sphere")
    assert adj.stats.cpu().numpy().tobytes() == ref[0].tobytes() and adj.start.cpu().numpy().tobytes() == ref[1].tobytes()
    assert adj.neighbours[:len(ref[2])].cpu().numpy().tobytes() == ref[2].tobytes() and ten.cpu().numpy().tobytes() == ref[5].tobytes()


def test_the_smoothing_property_holds_on_the_device():
    """the binary staircase sphere after 10 iterations at the defaults: the mean face-normal-to-radial angle below half the unsmoothed
    mesh's (the restatement: 20.65 deg -> 7.17 deg, ratio 0.347), the enclosed volume within 1 % (+ 0.35 %)"""
    v, f = sm.binary_sphere()
    ten = F.smooth_mesh(dev(v), dev(f)).cpu().numpy()                     # the defaults, the adjacency built from the faces
    assert ten.tobytes() == device_result("binary_sphere")[5].tobytes()
    before, after = sm.normal_angle_deg(v, f, sm.SPHERE_CENTRE), sm.normal_angle_deg(ten, f, sm.SPHERE_CENTRE)
    vol0, vol1 = sm.enclosed_volume(v, f), sm.enclosed_volume(ten, f)
    print(f"binary sphere on the device: angle {before:.2f} -> {after:.2f} deg (ratio {after / before:.3f}), volume {100 * (vol1 / vol0 - 1):+.2f} %")
    assert after < 0.5 * before
    assert abs(vol1 / vol0 - 1.0) < 0.01


def test_wrappers_refuse_what_they_cannot_take():
    v, f = sm.tetrahedron()
    tv, tf = dev(v), dev(f)
    adj = F.mesh_adjacency(tf, 4)
    assert F.mesh_topology(tf, 4).cpu().tolist() == sm.stats_row(sm.case("tetrahedron")[3]["stats"])
    for bad in (dict(iterations=-1), dict(iterations=10001), dict(iterations=2.5), dict(lam=0.0), dict(lam=1.5), dict(mu=0.5), dict(mu=-2.0),
                dict(lam=float("nan")), dict(mu=float("inf"))):
        with pytest.raises(L.GpnerfError):
            F.smooth_mesh(tv, adjacency=adj, **bad)
    with pytest.raises(L.GpnerfError):
        F.smooth_mesh(tv)                                                 # neither faces nor an adjacency
    with pytest.raises(L.GpnerfError):
        F.smooth_mesh(dev(np.zeros((5, 3), np.float32)), adjacency=adj)   # an adjacency of another mesh
    with pytest.raises(L.GpnerfError):
        F.smooth_mesh(tv, dev(f.astype(np.int64)))
    with pytest.raises(L.GpnerfError):
        F.smooth_mesh(dev(v.astype(np.float64)), tf)
    with pytest.raises(L.GpnerfError):
        F.mesh_adjacency(tf, -1)
    # a workspace that holds no finished adjacency of this many vertices: nothing is written
    lib = L.lib()
    ws = torch.zeros((int(lib.gpnerf_mesh_adjacency_workspace_bytes(4, 4)),), device=DEV, dtype=torch.uint8)
    out = torch.full((4, 3), 7.0, device=DEV)
    assert lib.gpnerf_mesh_smooth(tv.data_ptr(), 4, ws.data_ptr(), ws.numel(), 1, 0.5, -0.53, 1, out.data_ptr(), F._stream_ptr(torch.device(DEV))) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # in place: the first pass reads the caller's array, the last writes it
    again = tv.clone()
    assert lib.gpnerf_mesh_smooth(again.data_ptr(), 4, adj.workspace.data_ptr(), adj.workspace.numel(), 1, 0.5, -0.53, 1, again.data_ptr(),
                                  F._stream_ptr(torch.device(DEV))) == 0
    assert again.cpu().numpy().tobytes() == device_result("tetrahedron")[4].tobytes()


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    name = "mc_torus"
    v, f, pin, *_ = sm.case(name)
    lib = L.lib()
    tv, tf = dev(v), dev(f)
    nv, nf = len(v), len(f)
    ws = torch.zeros((int(lib.gpnerf_mesh_adjacency_workspace_bytes(nv, nf)),), device=DEV, dtype=torch.uint8)
    stats = torch.zeros((10,), device=DEV, dtype=torch.int64)
    out = torch.zeros((nv, 3), device=DEV)
    off = (__import__("ctypes").c_int64 * 3)()
    assert lib.gpnerf_mesh_adjacency_layout(nv, nf, off) == 0
    ref = device_result(name)

    def run():
        st = F._stream_ptr(torch.device(DEV))
        L.check(lib.gpnerf_mesh_adjacency(tf.data_ptr(), nf, nv, ws.data_ptr(), ws.numel(), stats.data_ptr(), st), "adjacency")
        return lib.gpnerf_mesh_smooth(tv.data_ptr(), nv, ws.data_ptr(), ws.numel(), sm.ITERATIONS, sm.LAM, sm.MU, 1 if pin else 0, out.data_ptr(), st)

    def outs():
        start = ws[off[0]:off[0] + 8 * (nv + 1)].view(torch.int64).cpu().numpy()
        nb = ws[off[1]:off[1] + 4 * int(start[-1])].view(torch.int32).cpu().numpy()
        return [stats.cpu().numpy().tobytes(), start.tobytes(), nb.tobytes(), ws[off[2]:off[2] + nv].cpu().numpy().tobytes(), out.cpu().numpy().tobytes()]

    assert run() == 0                                       # (also loads the kernels before the capture)
    torch.cuda.synchronize()
    first = outs()
    assert first == [ref[0].tobytes(), ref[1].tobytes(), ref[2].tobytes(), ref[3].tobytes(), ref[5].tobytes()]
    assert run() == 0
    torch.cuda.synchronize()
    assert outs() == first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert run() == 0
    for _ in range(2):
        stats.fill_(7)
        out.fill_(7)                                        # every output is written by the calls
        ws.fill_(0xAB)                                      # the workspace carries nothing into a call
        g.replay()
        torch.cuda.synchronize()
        assert outs() == first


def test_extract_mesh_smooths_behind_marching_cubes():
    """the binary sphere's cube through the lattice= route: the mesh is marching cubes', the vertices the restatement's after 3
    iterations, the normals are taken at them; topology alone leaves the mesh as it is; with both off no key is added"""
    g = np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing="ij"), -1).astype(np.float64)
    field = np.where(np.linalg.norm(g - sm.SPHERE_CENTRE, axis=-1) < 10.0, 0.04, 0.0).astype(np.float32)
    cube = torch.from_numpy(field).to(DEV)
    axes = [np.arange(32, dtype=np.float32) * np.float32(0.005)] * 3
    n_kept = torch.zeros((), device=DEV, dtype=torch.int64)
    vs = np.array([0.005, 0.005, 0.005])
    run = lambda **kw: F.extract_mesh(None, None, None, None, None, iso=0.02, host=[vs], lattice=(cube, axes, n_kept), **kw)
    plain = run()
    assert "topology_stats" not in plain and plain["faces"].shape[0] == 3784
    for off in (None, 0, "0", ""):
        m = run(smooth=off, topology=False)
        assert set(m) == set(plain) and m["vertices"].cpu().numpy().tobytes() == plain["vertices"].cpu().numpy().tobytes()
    topo = run(topology=True)
    assert set(topo) == set(plain) | {"topology_stats"} and topo["vertices"].cpu().numpy().tobytes() == plain["vertices"].cpu().numpy().tobytes()
    v, f = plain["vertices"].cpu().numpy(), plain["faces"].cpu().numpy()
    adj = sm.adjacency_np(f, len(v))
    assert topo["topology_stats"].cpu().tolist() == sm.stats_row(adj["stats"]) and F.read_mesh_topology(topo["topology_stats"])["watertight"]
    m = run(smooth=3, normals=True)
    assert m["topology_stats"].cpu().tolist() == sm.stats_row(adj["stats"]) and np.array_equal(m["faces"].cpu().numpy(), f)
    ov, n = m["vertices"].cpu().numpy(), m["normals"].cpu().numpy()
    assert ov.tobytes() == sm.smooth_np(v, adj, 3).tobytes() and ov.tobytes() != v.tobytes()
    assert n.tobytes() == F.mesh_normals(cube, m["vertices"], step=vs).cpu().numpy().tobytes()      # taken at the smoothed vertices
    assert n.tobytes() != run(normals=True)["normals"].cpu().numpy().tobytes()
    # behind simplify: the adjacency is the simplified mesh's
    both = run(simplify=2, smooth=2, topology=True)
    simple = run(simplify=2)
    sv, sf = simple["vertices"].cpu().numpy(), simple["faces"].cpu().numpy()
    sadj = sm.adjacency_np(sf, len(sv))
    assert both["topology_stats"].cpu().tolist() == sm.stats_row(sadj["stats"]) and np.array_equal(both["faces"].cpu().numpy(), sf)
    assert both["vertices"].cpu().numpy().tobytes() == sm.smooth_np(sv, sadj, 2).tobytes()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def renderers():
    p = os.path.join(ROOT, "gp-nerf_amd", "plugins")
    if p not in sys.path:
        sys.path.insert(0, p)
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
        off = make(mesh_smooth=0, mesh_topology=False).render_mesh(b)
        smooth = make(mesh_smooth=3, mesh_topology=True, mesh_normals=True, mesh_colors=True).render_mesh(b)
    return NS(base=base, off=off, smooth=smooth)


def test_render_mesh_with_the_knobs_off_is_todays(renderers):
    base, off = renderers.base, renderers.off
    assert set(off) == set(base) == {"mesh", "cube", "time_slots", "etime", "rtime"}
    assert set(off["time_slots"]) == set(base["time_slots"])
    assert off["cube"].tobytes() == base["cube"].tobytes()
    for name in ("vertices", "faces"):
        a, b = getattr(off["mesh"], name), getattr(base["mesh"], name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert off["mesh"].vertex_colors is None and off["mesh"].vertex_normals is None
    buf_a, buf_b = __import__("io").BytesIO(), __import__("io").BytesIO()
    off["mesh"].export(buf_a)
    base["mesh"].export(buf_b)
    assert buf_a.getvalue() == buf_b.getvalue()


def test_render_mesh_smooths_counts_colours_and_shades(renderers):
    base, smooth = renderers.base, renderers.smooth
    s = smooth["mesh_stats"]
    assert list(s) == list(L.TOPOLOGY_STATS) and len(s) == 10
    m = smooth["mesh"]
    v, f = base["mesh"].vertices.astype(np.float32), base["mesh"].faces
    assert np.array_equal(m.faces, f) and m.vertices.shape == v.shape
    adj = sm.adjacency_np(f, len(v))
    print("render_mesh(mesh_smooth=3, mesh_topology=True):", len(v), "vertices,", s)
    assert [s[k] for k in L.TOPOLOGY_STATS] == sm.stats_row(adj["stats"])
    assert s["faces_used"] == len(f) and s["faces_dropped"] == 0 and s["vertices_referenced"] == len(v)
    want = sm.smooth_np(v, adj, 3)
    got = m.vertices.astype(np.float32)
    print("render_mesh(mesh_smooth=3):", int((got.view(np.uint32) != want.view(np.uint32)).sum()), "of", want.size, "coordinates not bit-equal")
    assert got.tobytes() == want.tobytes() and got.tobytes() != v.tobytes()
    assert m.vertex_colors.shape == m.vertices.shape == m.vertex_normals.shape
    assert np.isfinite(m.vertex_colors).all() and m.vertex_colors.min() >= 0.0 and m.vertex_colors.max() <= 1.0
    norms = np.linalg.norm(m.vertex_normals.astype(np.float64), axis=1)
    assert np.isfinite(m.vertex_normals).all() and np.abs(norms[norms > 0.5] - 1.0).max() < 1e-5 and (norms > 0.5).mean() > 0.99


def test_mesh_evaluator_topology_end_to_end(tmp_path):
    """two frames -- a closed icosphere, the same with a face taken out --: a slot each, read once, the table and the means"""
    PAD = ev.MeshEvaluator.PAD
    v, f = mm.icosphere(2)
    v, f = np.asarray(v, dtype=np.float32) * 4.0 + 16.0, np.asarray(f, dtype=np.int32)
    cube = np.pad(np.zeros((13, 13, 13), np.float32), PAD)
    axes = [np.linspace(-0.6, 0.6, 13).astype(np.float32)] * 3
    meshes = [M.Mesh(v, f), M.Mesh(v, f[1:])]
    e = ev.MeshEvaluator(str(tmp_path / "a"), 0.02, topology=True)
    assert not e.has_mesh_metrics
    for i, mesh in enumerate(meshes):
        e.evaluate({"cube": cube, "mesh": mesh, "axes": axes}, {"frame_index": torch.tensor([10 + i])})
    assert e.has_mesh_metrics and len(e._topo_slots) == 2 and all(t.is_cuda for t in e._topo_slots)
    s = e.summarize()
    refs = [sm.adjacency_np(m.faces, len(v))["stats"] for m in meshes]
    assert s["watertight_frames"] == 1 and s["per_frame"]["watertight"] == [True, False] and s["per_frame"]["topology_frame_index"] == [10, 11]
    for k in ("edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "euler"):
        assert s["per_frame"][f"topology_{k}"] == [r[k] for r in refs] and s[f"topology_{k}"] == float(np.mean([r[k] for r in refs])), k
    assert s["per_frame"]["topology_boundary_edges"] == [0, 3] and s["per_frame"]["topology_euler"] == [2, 1]
    table = np.load(tmp_path / "a" / "topology_metrics.npy")
    assert len(table) == 2 and table["frame_index"].tolist() == [10, 11] and table["watertight"].tolist() == [True, False]
    for k in L.TOPOLOGY_STATS:
        assert table[k].tolist() == [r[k] for r in refs], k
    assert table["closed"].tolist() == [True, False] and table["oriented"].tolist() == [True, True]
    assert sorted(os.listdir(tmp_path / "a")) == ["pts", "topology_metrics.npy"]
    assert e.summarize() == {} and not e.has_mesh_metrics     # reset
    off = ev.MeshEvaluator(str(tmp_path / "b"), 0.02)
    off.evaluate({"cube": cube, "mesh": meshes[0], "axes": axes}, {"frame_index": torch.tensor([0])})
    assert not off.has_mesh_metrics and off.summarize() == {} and sorted(os.listdir(tmp_path / "b")) == ["pts"]
