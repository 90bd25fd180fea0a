"""GPU: the mesh repair (gpnerf_meshrepair.hip) against the numpy restatement of include/gpnerf_hip.h (tests/repair_cases.py): stats,
the five maps and the faces EQUAL, the output coordinates BIT-EQUAL to vertices[kept_vertices]; what each case is there for; a
shuffled face order changes no bit of the vertex outputs or the stats; two runs and a graph replay identical; an emit with a wrong
size writes nothing; with no flags the result is filter_components(keep=None)'s; MeshEvaluator(repair_gt=True) end to end.
Everything is integers and bit copies: every comparison is for equality."""
import functools
import importlib
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import mesh_metric_cases as mm
import repair_cases as rc
import smooth_cases as sm

pytestmark = pytest.mark.gpu
F = importlib.import_module("gp-nerf_amd.frame")
L = importlib.import_module("gp-nerf_amd._lib")
M = importlib.import_module("gp-nerf_amd.mesh")
ev = importlib.import_module("gp-nerf_amd.evaluator")
DEV = "cuda:0"
MAPS = ("vertex_map", "kept_vertices", "face_map", "face_fate", "face_patch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(v, f, kw):
    """frame.repair_mesh's outputs on the host"""
    ov, of, stats, maps = F.repair_mesh(dev(v), dev(f), want_map=True, **kw)
    host = lambda t: t.cpu().numpy()
    return {"vertices": host(ov), "faces": host(of), "stats": host(stats), **{k: host(getattr(maps, k)) for k in MAPS}}


@functools.lru_cache(maxsize=None)
def device_result(name):
    v, f, kw, _ref = rc.case(name)
    return run(v, f, kw)


def check(name):
    v, f, kw, ref = rc.case(name)
    got = device_result(name)
    print(name, dict(zip(L.REPAIR_STATS, got["stats"].tolist())))
    assert got["stats"].dtype == np.int64 and got["stats"].tolist() == rc.stats_row(ref["stats"])
    for k in MAPS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    assert got["faces"].dtype == np.int32 and got["faces"].shape == ref["faces"].shape and np.array_equal(got["faces"], ref["faces"])
    assert got["vertices"].dtype == np.float32 and got["vertices"].shape == (len(ref["kept_vertices"]), 3)
    assert got["vertices"].tobytes() == v[ref["kept_vertices"]].tobytes()                       # bit for bit
    return got, ref


@pytest.mark.parametrize("name", list(rc.CASES))
def test_the_repair_is_the_restatement(name):
    check(name)


def topology(v, f):
    return F.read_mesh_topology(F.mesh_topology(dev(f), len(v)))


def test_the_cases_reach_their_branches():
    row = lambda name: dict(zip(L.REPAIR_STATS, device_result(name)["stats"].tolist()))
    s = row("cube_soup")
    assert (s["vertices_out"], s["faces_out"], s["vertices_welded"], s["patches"], s["patches_closed"]) == (8, 12, 28, 1, 1)
    v, f = rc.case("cube_soup")[:2]
    cube = device_result("cube_soup")
    after = topology(cube["vertices"], cube["faces"])
    assert topology(v, f)["boundary_edges"] == 36 and after["watertight"] and after["euler"] == 2
    assert row("signed_zero")["vertices_out"] == 4 and row("signed_zero")["vertices_welded"] == 8
    nan = device_result("nan_vertex")
    assert row("nan_vertex")["vertices_unkeyable"] == 1 and (nan["face_fate"] == rc.UNKEYABLE).sum() == 3
    assert np.array_equal(nan["faces"][:4], sm.tetrahedron()[1]) and nan["vertices"][:4].tobytes() == sm.tetrahedron()[0].tobytes()
    g = device_result("grid")
    assert g["vertex_map"][0] != g["vertex_map"][1] and g["vertex_map"][2] == g["vertex_map"][3] and g["vertex_map"][7] == g["vertex_map"][8]
    assert g["vertex_map"][6] == -1 and row("grid")["vertices_unkeyable"] == 1
    group = rc.crowd()[2]
    lowest = np.array([np.nonzero(group == k)[0].min() for k in range(64)])
    crowd = device_result("crowd")
    assert np.array_equal(crowd["kept_vertices"], np.sort(lowest)) and np.array_equal(crowd["kept_vertices"][crowd["vertex_map"]], lowest[group])
    assert row("strip")["vertices_out"] > 2 * 2048 and row("strip")["faces_out"] > 2 * 2048        # the scans cross their blocks
    bad = device_result("bad_faces")
    assert bad["face_fate"].tolist()[-2:] == [rc.DUPLICATE] * 2 and bad["face_fate"][0] <= rc.KEPT_FLIPPED and row("bad_faces")["vertices_unreferenced"] == 2
    sphere = device_result("flipped_sphere")
    cv, cf = rc.ico(2)
    assert topology(sphere["vertices"], sphere["faces"])["inconsistent_edges"] == 0 and row("flipped_sphere")["faces_flipped"] == 160
    assert sphere["vertices"][sphere["faces"]].tobytes() == cv[cf].tobytes()
    s = row("inside_out")
    assert s["patches_inverted"] == 1 and s["faces_flipped"] == s["faces_out"] == 80
    untouched = device_result("inside_out_not_outward")
    assert row("inside_out_not_outward")["faces_flipped"] == 0 and np.array_equal(untouched["faces"], rc.case("inside_out_not_outward")[1])
    assert row("moebius")["patches_unorientable"] == 1 and np.array_equal(device_result("moebius")["faces"], rc.moebius()[1])
    clean = rc.sheet()[1]
    assert row("open_sheet_third")["faces_flipped"] == 96 and np.array_equal(device_result("open_sheet_third")["faces"], clean)
    assert row("open_sheet_half")["faces_flipped"] == 144 and np.array_equal(device_result("open_sheet_half")["faces"], clean)
    assert np.array_equal(device_result("open_sheet_half_root_flipped")["faces"], clean[:, [0, 2, 1]])     # the root's side stays
    s = row("shared_edge")
    assert (s["edges_nonmanifold"], s["patches"], s["patches_closed"], s["patches_inverted"], s["faces_flipped"]) == (1, 2, 2, 0, 0)
    assert row("flat_closed")["patches_undecided"] == 1 and row("flat_closed")["patches_closed"] == 1
    assert row("empty") == dict.fromkeys(L.REPAIR_STATS, 0) and row("no_faces")["vertices_unreferenced"] == 5
    assert device_result("no_faces")["vertex_map"].tolist() == [-1] * 5 and device_result("no_faces")["vertices"].shape == (0, 3)
    soup = device_result("mc_sphere_soup")
    top = topology(soup["vertices"], soup["faces"])
    assert top["watertight"] and top["euler"] == 2 and len(soup["vertices"]) == len(rc.mc_sphere_clean()[0])


def test_a_cavitys_wall_is_turned_and_the_parity_volume_stays():
    v, f = rc.case("nested")[:2]
    got = device_result("nested")
    assert dict(zip(L.REPAIR_STATS, got["stats"].tolist()))["patches_inverted"] == 1
    lattice = dict(lo=(-2.25, -2.25, -2.25), step=(0.1, 0.1, 0.1), dims=(46, 46, 46))
    grid = lambda vv, ff, rule: F.voxelize_mesh(dev(vv), dev(ff), rule=rule, **lattice)
    before, after = grid(v, f, "parity"), grid(got["vertices"], got["faces"], "parity")
    assert before.bits.cpu().numpy().tobytes() == after.bits.cpu().numpy().tobytes()
    hollow, filled = int(F.voxel_stats(after)[L.VOXEL_A]), int(F.voxel_stats(grid(got["vertices"], got["faces"], "nonzero"))[L.VOXEL_A])
    assert int(F.voxel_stats(grid(v, f, "nonzero"))[L.VOXEL_A]) == hollow < filled                # the nonzero rule now fills the cavity


@pytest.mark.parametrize("name", rc.ORDER_FREE)
def test_the_face_order_changes_no_bit_of_the_vertex_outputs_or_the_stats(name):
    v, f, kw, _ref = rc.case(name)
    g = sm.shuffled((v, f), seed=13)[1]
    assert not np.array_equal(f, g)
    x, y = device_result(name), run(v, g, kw)
    for k in ("stats", "vertices", "vertex_map", "kept_vertices"):
        assert x[k].tobytes() == y[k].tobytes(), k


def _raw(name):
    """the C calls on buffers of this test's own"""
    v, f, kw, ref = rc.case(name)
    lib = L.lib()
    tv, tf = dev(v), dev(f)
    nv, nf = len(v), len(f)
    flags = F._repair_flags(kw["weld"], kw["drop_duplicates"], kw["orient"], kw["outward"])
    ws = torch.zeros((int(lib.gpnerf_mesh_repair_workspace_bytes(nv, nf)),), device=DEV, dtype=torch.uint8)
    stats = torch.zeros((len(L.REPAIR_STATS),), device=DEV, dtype=torch.int64)
    n_v, n_f = ref["stats"]["vertices_out"], ref["stats"]["faces_out"]
    i32 = lambda n: torch.zeros((n,), device=DEV, dtype=torch.int32)
    out = NS(v=torch.zeros((n_v, 3), device=DEV), f=torch.zeros((n_f, 3), device=DEV, dtype=torch.int32), vertex_map=i32(nv), kept_vertices=i32(n_v),
             face_map=i32(n_f), face_fate=torch.zeros((nf,), device=DEV, dtype=torch.uint8), face_patch=i32(n_f))
    st = lambda: F._stream_ptr(torch.device(DEV))
    count = lambda: lib.gpnerf_mesh_repair(tv.data_ptr(), nv, tf.data_ptr(), nf, kw["tol"], flags, ws.data_ptr(), ws.numel(), stats.data_ptr(), st())
    emit = lambda n_out_v=n_v, n_out_f=n_f: lib.gpnerf_mesh_repair_emit(
        tv.data_ptr(), nv, tf.data_ptr(), nf, ws.data_ptr(), ws.numel(), out.v.data_ptr(), n_out_v, out.f.data_ptr(), n_out_f, out.vertex_map.data_ptr(),
        out.kept_vertices.data_ptr(), out.face_map.data_ptr(), out.face_fate.data_ptr(), out.face_patch.data_ptr(), st())
    tensors = [stats, out.v, out.f] + [getattr(out, k) for k in MAPS]
    outs = lambda: [t.cpu().numpy().tobytes() for t in tensors]
    status = lambda: int(ws[8 * L.REPAIR_HDR_STATUS:8 * L.REPAIR_HDR_STATUS + 8].view(torch.int64).item())
    return NS(count=count, emit=emit, outs=outs, status=status, ws=ws, tensors=tensors, sizes=(n_v, n_f))


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    name = "mc_sphere_soup"
    r = _raw(name)
    ref = device_result(name)
    assert r.count() == 0 and r.emit() == 0                 # (also loads the kernels before the capture)
    torch.cuda.synchronize()
    first = r.outs()
    assert first == [ref[k].tobytes() for k in ("stats", "vertices", "faces") + MAPS]
    assert r.count() == 0 and r.emit() == 0
    torch.cuda.synchronize()
    assert r.outs() == first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert r.count() == 0 and r.emit() == 0
    for _ in range(2):
        for t in r.tensors:
            t.fill_(7)                                      # every output is written by the calls
        r.ws.fill_(0xAB)                                    # the workspace carries nothing into a call
        g.replay()
        torch.cuda.synchronize()
        assert r.outs() == first and r.status() == L.REPAIR_EMITTED


def test_an_emit_with_a_wrong_size_writes_nothing():
    r = _raw("bad_faces")
    n_v, n_f = r.sizes
    assert r.count() == 0
    torch.cuda.synchronize()
    assert r.status() == L.REPAIR_COUNTED
    views = [t.view(-1).view(torch.uint8) for t in r.tensors[1:]]
    for wrong in ((n_v - 1, n_f), (n_v, n_f - 1), (n_v - 1, n_f - 1)):
        for t in views:
            t.fill_(0xAB)
        assert r.emit(*wrong) == 0
        torch.cuda.synchronize()
        assert r.status() == L.REPAIR_MISMATCH and all(bool((t == 0xAB).all()) for t in views), wrong
    assert r.emit() == 0                                    # the right sizes after a mismatch: a good emit
    torch.cuda.synchronize()
    ref = device_result("bad_faces")
    assert r.status() == L.REPAIR_EMITTED and r.outs() == [ref[k].tobytes() for k in ("stats", "vertices", "faces") + MAPS]
    r.ws.fill_(0)                                           # a workspace that holds no count: nothing is written either
    for t in views:
        t.fill_(0xAB)
    assert r.emit() == 0
    torch.cuda.synchronize()
    assert r.status() == L.REPAIR_NO_COUNT and all(bool((t == 0xAB).all()) for t in views)


@pytest.mark.parametrize("name", ["bad_faces_no_flags", "mc_sphere_no_flags"])
def test_with_no_flags_the_repair_is_keep_all(name):
    """the two "remove the rubbish" paths pinned to each other (meshes without an unkeyable vertex)"""
    v, f, kw, _ref = rc.case(name)
    got = device_result(name)
    ov, of, _stats, (vmap, kept) = F.filter_components(dev(v), dev(f), keep=None, want_map=True)
    assert got["vertices"].tobytes() == ov.cpu().numpy().tobytes() and got["faces"].tobytes() == of.cpu().numpy().tobytes()
    assert got["vertex_map"].tobytes() == vmap.cpu().numpy().tobytes() and got["kept_vertices"].tobytes() == kept.cpu().numpy().tobytes()
    assert got["stats"][9:].tolist() == [0] * 7


def test_wrappers_refuse_what_they_cannot_take():
    v, f = rc.case("cube_soup")[:2]
    tv, tf = dev(v), dev(f)
    for bad in (dict(tol=-1.0), dict(tol=float("nan")), dict(orient=False)):
        with pytest.raises(L.GpnerfError):
            F.repair_mesh(tv, tf, **bad)
    with pytest.raises(L.GpnerfError):
        F.repair_mesh(dev(v.astype(np.float64)), tf)
    with pytest.raises(L.GpnerfError):
        F.repair_mesh(tv, dev(f.astype(np.int64)))
    with pytest.raises(L.GpnerfError):
        F.repair_mesh(torch.from_numpy(v), torch.from_numpy(f))
    assert len(F.repair_mesh(tv, tf)) == 3 and len(F.repair_mesh(tv, tf, orient=False, outward=False, want_map=True)) == 4


def test_a_mesh_object_keeps_its_colours_and_its_atlas():
    """colours through kept_vertices, the atlas through face_map with a flipped face's UV rows swapped, the normals dropped"""
    v, f, kw, ref = rc.case("flipped_sphere")
    rng = np.random.default_rng(2)
    mesh = M.Mesh(v, f, vertex_colors=rng.uniform(size=(len(v), 3)).astype(np.float32), vertex_normals=v.copy(),
                  texture=rng.uniform(size=(4, 4, 3)).astype(np.float32), face_uvs=rng.uniform(size=(len(f), 3, 2)))
    out, stats = F.repair_mesh_object(mesh)
    assert stats == {**ref["stats"], "changed": True} and out.vertex_normals is None
    assert np.array_equal(out.faces, ref["faces"]) and out.vertices.astype(np.float32).tobytes() == ref["vertices"].tobytes()
    assert np.array_equal(out.vertex_colors, mesh.vertex_colors[ref["kept_vertices"]]) and np.array_equal(out.texture, mesh.texture)
    want = mesh.face_uvs[ref["face_map"]].copy()
    swap = ref["face_fate"][ref["face_map"]] == rc.KEPT_FLIPPED
    want[swap] = want[swap][:, [0, 2, 1]]
    assert swap.sum() == 160 and np.array_equal(out.face_uvs, want)
    soup, _ = F.repair_mesh_object(M.Mesh(*rc.case("cube_soup")[:2]), outward=False)
    assert len(soup.vertices) == 8 and soup.vertex_colors is None and soup.face_uvs is None


def test_mesh_evaluator_repairs_the_scan_before_any_metric(tmp_path):
    """a frame scored against the exploded, half-flipped scan with repair_gt=True gives exactly the numbers of the same frame scored
    against the restatement's repaired arrays with it off; off, on the clean scan, nothing of the repair appears"""
    PAD = ev.MeshEvaluator.PAD
    pv, pf = mm.icosphere(2)
    pred = M.Mesh(np.asarray(pv, dtype=np.float32) * 4.0 + 16.0, np.asarray(pf, dtype=np.int32))
    cube = np.pad(np.zeros((13, 13, 13), np.float32), PAD)
    axes = [np.linspace(-0.6, 0.6, 13).astype(np.float32)] * 3
    clean = rc.ico(2, 0.41)
    rng = np.random.default_rng(8)
    sv, sf = rc.explode(rc.flipped(clean, rng.permutation(320)[:160]))
    ref = rc.repair_np(sv, sf)
    assert ref["stats"]["faces_flipped"] == 160 and len(ref["vertices"]) == len(clean[0])
    knobs = dict(metric_samples=2000, volume=True, volume_rule="nonzero", signed=True)

    def score(path, gt, **kw):
        e = ev.MeshEvaluator(str(tmp_path / path), 0.02, **knobs, **kw)
        e.evaluate({"cube": cube, "mesh": pred, "axes": axes}, {"frame_index": torch.tensor([7]), "gt_mesh": gt})
        return e.summarize()

    on = score("on", M.Mesh(sv, sf), repair_gt=True)
    want = score("want", (ref["vertices"], ref["faces"]), repair_gt=False)
    ours = {k: v for k, v in on.items() if not k.startswith("gt_repair")}
    ours["per_frame"] = {k: v for k, v in on["per_frame"].items() if not k.startswith("gt_repair")}
    np.testing.assert_equal(ours, want)                     # (every key, every per-frame list; a NaN equals a NaN)
    assert want["volume_iou"] > 0.8
    assert on["gt_repaired_frames"] == 1 and on["per_frame"]["gt_repair_frame_index"] == [7]
    for k in L.REPAIR_STATS:
        assert on["per_frame"][f"gt_repair_{k}"] == [ref["stats"][k]], k
    assert on["per_frame"]["gt_repair_changed"] == [True]
    table = np.load(tmp_path / "on" / "repair_metrics.npy")
    assert table.dtype.names == ("frame_index",) + L.REPAIR_STATS + ("changed",) and table["frame_index"].tolist() == [7]
    assert table["vertices_welded"].tolist() == [960 - 162] and table["changed"].tolist() == [True]
    assert sorted(set(os.listdir(tmp_path / "on")) - set(os.listdir(tmp_path / "want"))) == ["repair_metrics.npy"]
    # the broken scan without the repair scores differently: the knob is what made the numbers right
    broken = score("broken", M.Mesh(sv, sf))
    assert broken["volume_iou"] != want["volume_iou"]
    # off, on the clean scan: no key, no file, the numbers of an evaluator that was never given the keyword
    off = score("off", M.Mesh(*clean), repair_gt=False)
    plain = score("plain", M.Mesh(*clean))
    np.testing.assert_equal(off, plain)
    assert not any("repair" in k for k in list(off) + list(off["per_frame"]))
    assert sorted(os.listdir(tmp_path / "off")) == sorted(os.listdir(tmp_path / "plain")) and "repair_metrics.npy" not in os.listdir(tmp_path / "off")
