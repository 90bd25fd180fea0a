"""GPU: the mesh's connected components (gpnerf_meshcomp.hip) against the numpy restatement of include/gpnerf_hip.h
(tests/component_cases.py): labels, numbers, the table's defined rows and the stats EQUAL; the emitted mesh equal, its coordinates
BIT-EQUAL to the kept inputs; a shuffled face order changes no bit of labels, table or stats; two runs and a graph replay identical;
an emit with a wrong size writes nothing; extract_mesh(components=), Renderer(mesh_components=) and MeshEvaluator(components=True) end
to end.  Everything is integers and bit copies: every comparison is for equality."""
import ctypes as C
import functools
import importlib
import os
import sys
import types
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import component_cases as cc
import mesh_metric_cases as mm
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
KEEPS = {cc.KEEP_ALL: None, cc.KEEP_LARGEST: "largest"}
SCENE_SELECTIONS = [(cc.KEEP_ALL, 1), (cc.KEEP_LARGEST, 1)] + [(cc.KEEP_MIN_FACES, n) for n in (80, 81, 336, 337, 600, 601)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def device_result(name, keep=cc.KEEP_ALL, min_faces=1):
    """the device's outputs on the host: dict of label, vertex_component, face_component, table (the first C rows), stats, and the
    emitted vertices, faces, vertex_map, kept_vertices"""
    v, f = cc.mesh(name)
    tv, tf = dev(v), dev(f)
    comp = F.mesh_components(tf, len(v), keep=min_faces if keep == cc.KEEP_MIN_FACES else KEEPS[keep])
    assert comp.label.shape == comp.vertex_component.shape == (len(v),) and comp.face_component.shape == (len(f),)
    assert comp.table.shape == (len(v) // 3, 6) and comp.stats.shape == (9,) and (comp.keep, comp.n_vertices, comp.n_faces) == (keep, len(v), len(f))
    ov, of, stats, (vmap, kept) = F.filter_components(tv, tf, components=comp, want_map=True)
    assert stats is comp.stats
    torch.cuda.synchronize()
    status = int(comp.workspace[8 * L.COMPONENTS_HDR_STATUS:8 * L.COMPONENTS_HDR_STATUS + 8].view(torch.int64).item())
    host = lambda t: t.cpu().numpy()
    s = host(comp.stats)
    return {"label": host(comp.label), "vertex_component": host(comp.vertex_component), "face_component": host(comp.face_component),
            "table": host(comp.table)[:int(s[0])], "stats": s, "vertices": host(ov), "faces": host(of), "vertex_map": host(vmap),
            "kept_vertices": host(kept), "status": status}


def check(name, keep=cc.KEEP_ALL, min_faces=1):
    v, f, ref = cc.case(name, keep, min_faces)
    got = device_result(name, keep, min_faces)
    print(name, keep, min_faces, dict(zip(L.COMPONENT_STATS, got["stats"].tolist())))
    assert got["stats"].dtype == np.int64 and got["stats"].tolist() == cc.stats_row(ref["stats"])
    for k in ("label", "vertex_component", "face_component"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k
    assert got["table"].dtype == np.int64 and np.array_equal(got["table"], ref["table"])
    assert got["status"] == L.COMPONENTS_EMITTED
    assert got["kept_vertices"].dtype == np.int32 and np.array_equal(got["kept_vertices"], ref["kept_vertices"])
    assert got["vertex_map"].dtype == np.int32 and np.array_equal(got["vertex_map"], ref["vertex_map"])
    assert got["faces"].dtype == np.int32 and got["faces"].shape == ref["out_faces"].shape and np.array_equal(got["faces"], ref["out_faces"])
    assert got["vertices"].dtype == np.float32 and got["vertices"].tobytes() == v[ref["kept_vertices"]].tobytes()       # bit for bit
    # the two maps are inverse to each other
    assert np.array_equal(got["vertex_map"][got["kept_vertices"]], np.arange(len(got["kept_vertices"])))
    assert np.array_equal(np.nonzero(got["vertex_map"] >= 0)[0], got["kept_vertices"])
    return got, ref


@pytest.mark.parametrize("name", list(cc.CASES))
def test_components_are_the_restatement(name):
    check(name)


@pytest.mark.parametrize("name", ["bad_faces", "two_tetrahedra", "twin_blobs", "noise", "strip", "empty", "no_faces"])
def test_keeping_the_largest_is_the_restatement(name):
    got, ref = check(name, cc.KEEP_LARGEST)
    assert got["stats"][6] == (1 if ref["stats"]["components"] else 0)


def test_the_cases_reach_their_branches():
    row = lambda name, *sel: dict(zip(L.COMPONENT_STATS, device_result(name, *sel)["stats"].tolist()))
    assert row("bow_tie")["components"] == 1                                      # vertex connectivity
    two = device_result("two_tetrahedra")
    assert two["label"].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, -1] and two["table"][:, 0].tolist() == [0, 1] and two["vertex_map"][8] == -1
    assert row("twin_blobs")["largest"] == 0 and device_result("twin_blobs")["table"][:, 3].tolist() == [928, 928]       # the tie: the lower number
    assert device_result("twin_blobs", cc.KEEP_LARGEST)["faces"].shape == (928, 3)
    assert row("noise")["components"] == 263 and row("noise")["largest_faces"] == 105824 and device_result("noise")["table"][0, 0] == 0
    assert row("strip")["components"] == 1 and row("hub_last_fan")["components"] == 1 and len(cc.mesh("strip")[0]) > 2 * 2048          # (the vertices cross the scan's blocks)
    assert row("empty")["largest"] == -1 and row("no_faces")["kept_vertices"] == 0 and device_result("no_faces")["vertex_map"].tolist() == [-1] * 5
    assert device_result("scene")["table"][:, 3].tolist() == [600, 600, 5472, 944, 236, 336, 80]


@pytest.mark.parametrize("keep,min_faces", SCENE_SELECTIONS)
def test_the_scenes_selections_are_the_restatement(keep, min_faces):
    got, ref = check("scene", keep, min_faces)
    assert len(got["faces"]) == ref["stats"]["kept_faces"]
    if keep == cc.KEEP_LARGEST:
        # the emitted mesh's own topology: the torus, watertight, one component of genus 1
        tf = dev(got["faces"])
        adj = F.mesh_adjacency(tf, len(got["vertices"]))
        topo = F.read_mesh_topology(adj.stats)
        assert topo["watertight"] and topo["euler"] == 0 and topo["faces_used"] == 5472 and topo["vertices_referenced"] == len(got["vertices"])
        again = F.mesh_components(tf, len(got["vertices"]), adjacency=adj)
        res = F.read_mesh_components(again.stats, again.table, adj.stats)
        assert res["components"] == 1 and res["largest_genus"] == 1 and res["rows"][0]["closed"]


def test_the_genus_of_every_piece_of_the_scene():
    v, f = cc.mesh("scene")
    comp = F.mesh_components(dev(f), len(v))
    res = F.read_mesh_components(comp.stats, comp.table, comp.adjacency.stats)
    assert [r["genus"] for r in res["rows"]] == [0, 0, 1, 0, 0, 0, 0] and res["closed_components"] == 7 and res["largest_genus"] == 1
    v, f = cc.mesh("noise")
    comp = F.mesh_components(dev(f), len(v))
    res = F.read_mesh_components(comp.stats, comp.table, comp.adjacency.stats)
    assert all(r["genus"] is None for r in res["rows"])                   # non-manifold edges: no genus is vouched for


def test_the_face_order_changes_no_bit_of_labels_table_or_stats():
    for a, b in (("scene", "scene_shuffled"), ("two_tetrahedra", "two_tetrahedra_shuffled")):
        assert not np.array_equal(cc.mesh(a)[1], cc.mesh(b)[1])
        x, y = device_result(a), device_result(b)
        for k in ("label", "vertex_component", "table", "stats", "vertices", "vertex_map", "kept_vertices"):
            assert x[k].tobytes() == y[k].tobytes(), (a, k)
    v, f = cc.mesh("noise")
    _v, g = sm.shuffled((v, f), seed=9)
    comp = F.mesh_components(dev(g), len(v), keep="largest")
    ref = device_result("noise", cc.KEEP_LARGEST)
    assert comp.label.cpu().numpy().tobytes() == ref["label"].tobytes() and comp.stats.cpu().numpy().tobytes() == ref["stats"].tobytes()
    assert comp.table[:263].cpu().numpy().tobytes() == ref["table"].tobytes()


def _raw(name, keep, min_faces):
    """the C calls on buffers of this test's own: (run, outs, buffers)"""
    v, f = cc.mesh(name)
    lib = L.lib()
    tv, tf = dev(v), dev(f)
    nv, nf = len(v), len(f)
    adj = F.mesh_adjacency(tf, nv)
    ws = torch.zeros((int(lib.gpnerf_mesh_components_workspace_bytes(nv, nf)),), device=DEV, dtype=torch.uint8)
    stats = torch.zeros((9,), device=DEV, dtype=torch.int64)
    off = (C.c_int64 * 4)()
    assert lib.gpnerf_mesh_components_layout(nv, nf, off) == 0
    ref = cc.case(name, keep, min_faces)[2]
    n_v, n_f = ref["stats"]["kept_vertices"], ref["stats"]["kept_faces"]
    out = NS(v=torch.zeros((n_v, 3), device=DEV), f=torch.zeros((n_f, 3), device=DEV, dtype=torch.int32),
             vmap=torch.zeros((nv,), device=DEV, dtype=torch.int32), kept=torch.zeros((n_v,), device=DEV, dtype=torch.int32))
    st = lambda: F._stream_ptr(torch.device(DEV))

    def count():
        return lib.gpnerf_mesh_components(tf.data_ptr(), nf, nv, adj.workspace.data_ptr(), adj.workspace.numel(), keep, min_faces, ws.data_ptr(),
                                          ws.numel(), stats.data_ptr(), st())

    def emit(n_out_v=n_v, n_out_f=n_f):
        return lib.gpnerf_mesh_components_emit(tv.data_ptr(), nv, tf.data_ptr(), nf, ws.data_ptr(), ws.numel(), n_out_v, n_out_f, out.v.data_ptr(),
                                               out.f.data_ptr(), out.vmap.data_ptr(), out.kept.data_ptr(), st())

    def outs():
        c = int(stats[0].item())
        view = lambda o, n: ws[o:o + n].cpu().numpy().tobytes()
        return [stats.cpu().numpy().tobytes(), view(off[0], 4 * nv), view(off[1], 4 * nv), view(off[2], 4 * nf), view(off[3], 48 * c)] + \
               [t.cpu().numpy().tobytes() for t in (out.v, out.f, out.vmap, out.kept)]

    status = lambda: int(ws[8 * L.COMPONENTS_HDR_STATUS:8 * L.COMPONENTS_HDR_STATUS + 8].view(torch.int64).item())
    return NS(count=count, emit=emit, outs=outs, status=status, ws=ws, stats=stats, out=out, adj=adj, sizes=(nv, nf, n_v, n_f), tf=tf)


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    name, keep, n_min = "scene", cc.KEEP_MIN_FACES, 336
    r = _raw(name, keep, n_min)
    ref = device_result(name, keep, n_min)
    assert r.count() == 0 and r.emit() == 0                 # (also loads the kernels before the capture)
    torch.cuda.synchronize()
    first = r.outs()
    assert first == [ref[k].tobytes() for k in ("stats", "label", "vertex_component", "face_component", "table", "vertices", "faces",
                                                "vertex_map", "kept_vertices")]
    assert r.count() == 0 and r.emit() == 0
    torch.cuda.synchronize()
    assert r.outs() == first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert r.count() == 0 and r.emit() == 0
    for _ in range(2):
        r.stats.fill_(7)
        for t in (r.out.v, r.out.f, r.out.vmap, r.out.kept):
            t.fill_(7)                                      # every output is written by the calls
        r.ws.fill_(0xAB)                                    # the workspace carries nothing into a call
        g.replay()
        torch.cuda.synchronize()
        assert r.outs() == first and r.status() == L.COMPONENTS_EMITTED


def test_an_emit_with_a_wrong_size_writes_nothing():
    r = _raw("scene", cc.KEEP_LARGEST, 1)
    nv, nf, n_v, n_f = r.sizes
    assert r.count() == 0
    torch.cuda.synchronize()
    assert r.status() == L.COMPONENTS_COUNTED
    views = [t.view(torch.uint8) for t in (r.out.v.view(-1), r.out.f.view(-1), r.out.vmap, r.out.kept)]
    for wrong in ((n_v - 1, n_f), (n_v, n_f - 1), (n_v - 1, n_f - 1)):
        for t in views:
            t.fill_(0xAB)
        assert r.emit(*wrong) == 0
        torch.cuda.synchronize()
        assert r.status() == L.COMPONENTS_MISMATCH and all(bool((t == 0xAB).all()) for t in views), wrong
    assert r.emit() == 0                                    # the right sizes after a mismatch: a good emit
    torch.cuda.synchronize()
    ref = device_result("scene", cc.KEEP_LARGEST)
    assert r.status() == L.COMPONENTS_EMITTED and r.out.f.cpu().numpy().tobytes() == ref["faces"].tobytes()
    assert r.out.v.cpu().numpy().tobytes() == ref["vertices"].tobytes()
    # a workspace that holds no count: nothing is written either
    r.ws.fill_(0)
    for t in views:
        t.fill_(0xAB)
    assert r.emit() == 0
    torch.cuda.synchronize()
    assert all(bool((t == 0xAB).all()) for t in views)


def test_without_a_finished_adjacency_nothing_is_written():
    r = _raw("tetrahedron", cc.KEEP_ALL, 1)
    lib = L.lib()
    nv, nf = 4, 4
    blank = torch.zeros_like(r.adj.workspace)
    other = F.mesh_adjacency(dev(cc.mesh("two_tetrahedra")[1]), 9)       # a finished adjacency of ANOTHER mesh, large enough
    assert other.workspace.numel() >= r.adj.workspace.numel()
    for aws in (blank, other.workspace):
        r.stats.fill_(7)
        r.ws.fill_(0xAB)
        assert lib.gpnerf_mesh_components(r.tf.data_ptr(), nf, nv, aws.data_ptr(), aws.numel(), 0, 0, r.ws.data_ptr(), r.ws.numel(),
                                          r.stats.data_ptr(), F._stream_ptr(torch.device(DEV))) == 0
        assert r.emit() == 0
        torch.cuda.synchronize()
        assert r.status() == L.COMPONENTS_NO_ADJACENCY and bool((r.stats == 7).all())
        off = (C.c_int64 * 4)()
        assert lib.gpnerf_mesh_components_layout(nv, nf, off) == 0
        for o, n in ((off[0], 4 * nv), (off[1], 4 * nv), (off[2], 4 * nf), (off[3], 48)):
            assert bool((r.ws[o:o + n] == 0xAB).all())
        assert bool((r.out.vmap == 0).all())                # emit wrote nothing
    assert r.count() == 0 and r.emit() == 0
    torch.cuda.synchronize()
    assert r.status() == L.COMPONENTS_EMITTED and r.stats.cpu().tolist() == cc.stats_row(cc.case("tetrahedron")[2]["stats"])


def test_wrappers_refuse_what_they_cannot_take():
    v, f = cc.mesh("two_tetrahedra")
    tv, tf = dev(v), dev(f)
    adj = F.mesh_adjacency(tf, len(v))
    for bad in (dict(keep="smallest"), dict(keep=-2), dict(keep=2.5), dict(min_faces=0), dict(keep="largest", min_faces=3), dict(min_faces=True)):
        with pytest.raises(L.GpnerfError):
            F.mesh_components(tf, len(v), adjacency=adj, **bad)
    with pytest.raises(L.GpnerfError):
        F.mesh_components(tf, 8, adjacency=adj)                              # an adjacency of another vertex count
    with pytest.raises(L.GpnerfError):
        F.mesh_components(dev(f.astype(np.int64)), len(v))
    with pytest.raises(L.GpnerfError):
        F.filter_components(dev(v.astype(np.float64)), tf)
    with pytest.raises(L.GpnerfError):
        F.filter_components(tv[:5].contiguous(), tf, components=F.mesh_components(tf, len(v)))
    # the ways to say a selection agree
    a = F.mesh_components(tf, len(v), adjacency=adj, keep=4).stats.cpu().tolist()
    b = F.mesh_components(tf, len(v), adjacency=adj, min_faces=4).stats.cpu().tolist()
    assert a == b == [2, 2, 0, 4, 4, 2, 2, 8, 8]
    assert F.mesh_components(tf, len(v), keep=5).stats.cpu().tolist()[6:] == [0, 0, 0]
    ov, of, stats, maps = F.filter_components(tv, tf, keep=5)                # nothing is kept: empty outputs
    assert ov.shape == (0, 3) and of.shape == (0, 3) and maps is None
    ov, of, stats, maps = F.filter_components(tv, tf)                        # the default: the largest
    assert of.cpu().numpy().tolist() == (sm.tetrahedron()[1]).tolist() and ov.cpu().numpy().tobytes() == v[0:8:2].tobytes()


def test_extract_mesh_filters_behind_marching_cubes():
    """the scene's field through the lattice= route: with components the mesh is the restatement's selection of marching cubes' mesh,
    topology and normals are of the mesh as returned; off, no key is added and no bit changes"""
    shape = (48, 48, 48)
    field = __import__("mesh_cases").torus_field(48, 12.0, 4.0)
    for centre, r in (((8.31, 8.17, 8.07), 4.0), ((8.31, 8.17, 40.07), 4.0), ((40.2, 8.3, 40.1), 3.0), ((40.3, 40.2, 8.4), 1.5)):
        field = np.maximum(field, cc.ball_field(shape, centre, r))
    field = np.maximum(field, cc.shell_field(shape, (23.73, 23.73, 23.73), 2.5, 5.0))
    cube = torch.from_numpy(field).to(DEV)
    axes = [np.arange(48, dtype=np.float32) * np.float32(0.005)] * 3
    n_kept = torch.zeros((), device=DEV, dtype=torch.int64)
    vs = np.array([0.005, 0.005, 0.005])
    run = lambda **kw: F.extract_mesh(None, None, None, None, None, iso=0.02, host=[vs], lattice=(cube, axes, n_kept), **kw)
    plain = run()
    v, f = plain["vertices"].cpu().numpy(), plain["faces"].cpu().numpy()
    assert "component_stats" not in plain and len(f) == len(cc.mesh("scene")[1]) and len(v) == len(cc.mesh("scene")[0])
    adjacency, label = sm.adjacency_np(f, len(v)), cc.labels_np(f, len(v))
    for off in (None, 0, "0", "", False):
        m = run(components=off)
        assert set(m) == set(plain) and m["vertices"].cpu().numpy().tobytes() == v.tobytes() and np.array_equal(m["faces"].cpu().numpy(), f)
    for knob, sel in (("largest", (cc.KEEP_LARGEST, 1)), (337, (cc.KEEP_MIN_FACES, 337)), ("81", (cc.KEEP_MIN_FACES, 81))):
        ref = cc.components_np(f, len(v), *sel, adjacency=adjacency, label=label)      # of the device's own marching-cubes mesh
        assert ref["stats"]["kept_faces"] == cc.case("scene", *sel)[2]["stats"]["kept_faces"]
        m = run(components=knob, topology=True, normals=True)
        assert set(m) == set(plain) | {"component_stats", "topology_stats", "normals"}
        assert m["component_stats"].cpu().tolist() == cc.stats_row(ref["stats"])
        ov, of = m["vertices"].cpu().numpy(), m["faces"].cpu().numpy()
        assert np.array_equal(of, ref["out_faces"]) and ov.tobytes() == v[ref["kept_vertices"]].tobytes()
        assert m["topology_stats"].cpu().tolist() == sm.stats_row(sm.adjacency_np(of, len(ov))["stats"])        # of the mesh as returned
        assert m["normals"].shape == m["vertices"].shape
        assert m["normals"].cpu().numpy().tobytes() == F.mesh_normals(cube, m["vertices"], step=vs).cpu().numpy().tobytes()
    # behind simplify and in front of smoothing
    both = run(simplify=2, components="largest", smooth=2)
    simple = run(simplify=2)
    sv, sf = simple["vertices"].cpu().numpy(), simple["faces"].cpu().numpy()
    ref = cc.components_np(sf, len(sv), cc.KEEP_LARGEST)
    assert both["component_stats"].cpu().tolist() == cc.stats_row(ref["stats"]) and np.array_equal(both["faces"].cpu().numpy(), ref["out_faces"])
    kept_v = sv[ref["kept_vertices"]]
    assert both["vertices"].cpu().numpy().tobytes() == sm.smooth_np(kept_v, sm.adjacency_np(ref["out_faces"], len(kept_v)), 2).tobytes()
    with pytest.raises(L.GpnerfError):
        run(components="smallest")


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
        base = make(mesh_colors=False, mesh_clean=0, mesh_normals=False, mesh_simplify=0, mesh_smooth=0, mesh_topology=False,
                    mesh_components=0).render_mesh(b)
        off = make(mesh_components=0).render_mesh(b)
        default = plain.render_mesh(b)
        largest = make(mesh_components="largest", mesh_topology=True).render_mesh(b)
    return NS(base=base, off=off, default=default, largest=largest)


def test_render_mesh_with_the_knob_off_is_the_render_with_every_mesh_knob_off(renderers):
    for other in (renderers.off, renderers.default):
        base = renderers.base
        assert set(other) == set(base) == {"mesh", "cube", "time_slots", "etime", "rtime"}
        assert other["cube"].tobytes() == base["cube"].tobytes()
        for name in ("vertices", "faces"):
            a, b = getattr(other["mesh"], name), getattr(base["mesh"], name)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
        buf_a, buf_b = __import__("io").BytesIO(), __import__("io").BytesIO()
        other["mesh"].export(buf_a)
        base["mesh"].export(buf_b)
        assert buf_a.getvalue() == buf_b.getvalue()


def test_render_mesh_keeps_the_largest_component_of_the_body(renderers):
    base, largest = renderers.base, renderers.largest
    v, f = base["mesh"].vertices.astype(np.float32), base["mesh"].faces
    ref = cc.components_np(f, len(v), cc.KEEP_LARGEST)
    s = largest["mesh_stats"]
    print("render_mesh(mesh_components='largest'):", len(v), "vertices,", len(f), "faces,", {k: s[k] for k in s if k.startswith("mesh_")})
    assert [s[f"mesh_{k}"] for k in L.COMPONENT_STATS] == cc.stats_row(ref["stats"])
    assert s["mesh_components"] > 1 and sm.adjacency_np(f, len(v))["stats"]["euler"] == 84         # the body cube's floaters
    m = largest["mesh"]
    assert np.array_equal(m.faces, ref["out_faces"]) and m.vertices.astype(np.float32).tobytes() == v[ref["kept_vertices"]].tobytes()
    # the topology counts are the filtered mesh's, and it is one component
    after = sm.adjacency_np(m.faces, len(m.vertices))
    assert [s[k] for k in L.TOPOLOGY_STATS] == sm.stats_row(after["stats"])
    assert cc.components_np(m.faces, len(m.vertices), adjacency=after)["stats"]["components"] == 1
    again = F.mesh_components(dev(m.faces.astype(np.int32)), len(m.vertices))
    assert again.stats.cpu().tolist()[0] == 1


def test_mesh_evaluator_components_end_to_end(tmp_path):
    """three frames -- a closed icosphere, two of them apart, the sphere with a face taken out --: a slot each, read once"""
    PAD = ev.MeshEvaluator.PAD
    v, f = mm.icosphere(2)
    v, f = np.asarray(v, dtype=np.float32) * 4.0 + 16.0, np.asarray(f, dtype=np.int32)
    cube = np.pad(np.zeros((13, 13, 13), np.float32), PAD)
    axes = [np.linspace(-0.6, 0.6, 13).astype(np.float32)] * 3
    meshes = [M.Mesh(v, f), M.Mesh(np.concatenate([v, v + np.float32(20.0)]), np.concatenate([f, f[:-2] + len(v)])), M.Mesh(v, f[1:])]
    e = ev.MeshEvaluator(str(tmp_path / "a"), 0.02, components=True)
    assert not e.has_mesh_metrics
    for i, mesh in enumerate(meshes):
        e.evaluate({"cube": cube, "mesh": mesh, "axes": axes}, {"frame_index": torch.tensor([10 + i])})
    assert e.has_mesh_metrics and len(e._comp_slots) == 3 and all(t.is_cuda for t in e._comp_slots)
    s = e.summarize()
    refs = [cc.components_np(m.faces, len(m.vertices))["stats"] for m in meshes]
    assert [r["components"] for r in refs] == [1, 2, 1]
    assert s["components_mean"] == 4.0 / 3.0 and s["single_component_frames"] == 2
    assert s["per_frame"]["components"] == [1, 2, 1] and s["per_frame"]["components_frame_index"] == [10, 11, 12]
    assert s["per_frame"]["components_largest_faces"] == [len(f), len(f), len(f) - 1]
    assert s["per_frame"]["components_largest_genus"] == [0, 0, -1]           # the open sphere has no genus
    table = np.load(tmp_path / "a" / "components_metrics.npy")
    assert table.dtype.names == ("frame_index",) + L.COMPONENT_STATS + ("largest_genus",)
    assert table["frame_index"].tolist() == [10, 11, 12] and table["largest_genus"].tolist() == [0, 0, -1]
    for k in L.COMPONENT_STATS:
        assert table[k].tolist() == [r[k] for r in refs], k
    assert sorted(os.listdir(tmp_path / "a")) == ["components_metrics.npy", "pts"]
    assert e.summarize() == {} and not e.has_mesh_metrics     # reset
    # topology=True alone is what it was: its keys, its file, and nothing of the components
    t = ev.MeshEvaluator(str(tmp_path / "b"), 0.02, topology=True)
    t.evaluate({"cube": cube, "mesh": meshes[0], "axes": axes}, {"frame_index": torch.tensor([0])})
    st = t.summarize()
    assert not any("component" in k for k in list(st) + list(st["per_frame"])) and sorted(os.listdir(tmp_path / "b")) == ["pts", "topology_metrics.npy"]
    off = ev.MeshEvaluator(str(tmp_path / "c"), 0.02)
    off.evaluate({"cube": cube, "mesh": meshes[0], "axes": axes}, {"frame_index": torch.tensor([0])})
    assert not off.has_mesh_metrics and off.summarize() == {} and sorted(os.listdir(tmp_path / "c")) == ["pts"]
