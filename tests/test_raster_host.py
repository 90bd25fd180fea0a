"""CPU: the rasteriser's entry points refuse bad arguments on the host before anything is launched, the workspace formula, the
wrappers refuse CPU tensors, and self-checks of the numpy restatement (tests/raster_cases.py) the GPU tests compare against."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import hull_cases
import mesh_metric_cases as mm
import raster_cases as rc

P = 0x1000                                                   # a non-null dummy: argument checks never dereference


def _cams(n=1):
    return np.ascontiguousarray(np.tile(np.concatenate([np.eye(3).ravel(), np.eye(3, 4).ravel()]), (n, 1)))


def test_rasterize_rejects_bad_arguments_on_the_host(pkg):
    L = pkg._lib
    lib = L.lib()
    cams = _cams(8).ctypes.data_as(L.DP)
    big = 1 << 40

    def call(vertices=P, nv=10, faces=P, nf=5, cams=cams, n_views=3, H=24, W=40, z_near=1e-6, ws=P, ws_bytes=big):
        return lib.gpnerf_mesh_rasterize(vertices, nv, faces, nf, cams, n_views, H, W, z_near, ws, ws_bytes, P, P, P, None)

    for bad in (dict(vertices=None), dict(faces=None), dict(cams=None), dict(ws=None), dict(n_views=0), dict(n_views=9), dict(H=0), dict(W=0),
                dict(H=-3), dict(W=16385), dict(z_near=0.0), dict(z_near=-1.0), dict(z_near=float("nan")), dict(z_near=float("inf")),
                dict(nv=-1), dict(nf=-1), dict(nf=1 << 31)):
        assert call(**bad) == -1, bad
    need = int(lib.gpnerf_mesh_raster_workspace_bytes(5, 3, 24, 40))
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1


def test_interpolate_and_silhouette_reject_bad_arguments_on_the_host(pkg):
    L = pkg._lib
    lib = L.lib()
    cams = _cams(8).ctypes.data_as(L.DP)
    bg = (C.c_float * 4)(0, 0, 0, 0)

    def interp(face_id=P, vertices=P, nv=10, faces=P, nf=5, cams=cams, n_views=3, H=24, W=40, z_near=1e-6, attrs=P, c=3, bg=bg, out=P):
        return lib.gpnerf_mesh_interpolate(face_id, vertices, nv, faces, nf, cams, n_views, H, W, z_near, attrs, c, bg, out, None)

    for bad in (dict(face_id=None), dict(vertices=None), dict(faces=None), dict(cams=None), dict(attrs=None), dict(bg=None), dict(out=None),
                dict(c=0), dict(c=5), dict(n_views=0), dict(n_views=9), dict(H=0), dict(W=0), dict(z_near=0.0), dict(nf=-1)):
        assert interp(**bad) == -1, bad

    def sil(face_id=P, masks=P, n_views=3, H=24, W=40, out=P):
        return lib.gpnerf_silhouette_stats(face_id, masks, n_views, H, W, out, None)

    for bad in (dict(face_id=None), dict(masks=None), dict(out=None), dict(n_views=0), dict(n_views=9), dict(H=0), dict(W=0)):
        assert sil(**bad) == -1, bad


def test_the_workspace_formula(pkg):
    """include/gpnerf_hip.h: 256 + align256(8 V H W) + align256(8 n_faces V): the header, a 64-bit key per pixel and view, a list entry
    per (face, view) pair at worst; host arithmetic only; 0 for what the call refuses"""
    lib = pkg._lib.lib()
    ws = lambda nf, v, h, w: int(lib.gpnerf_mesh_raster_workspace_bytes(nf, v, h, w))
    al = lambda b: (b + 255) // 256 * 256
    for nf, v, h, w in ((0, 1, 1, 1), (1, 1, 24, 40), (5120, 3, 70, 130), (400000, 3, 1024, 1024), (7, 8, 16384, 16384), (2 ** 31 - 1, 8, 5, 3)):
        assert ws(nf, v, h, w) == 256 + al(8 * v * h * w) + al(8 * nf * v), (nf, v, h, w)
    for refused in ((-1, 1, 4, 4), (1 << 31, 1, 4, 4), (5, 0, 4, 4), (5, 9, 4, 4), (5, 1, 0, 4), (5, 1, 4, 0), (5, 1, 16385, 4)):
        assert ws(*refused) == 0, refused


def test_cpu_tensors_are_refused(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    v, f = mm.one_triangle()
    Ks, RTs = rc.pixel_cameras(1)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.rasterize_mesh(torch.from_numpy(v), torch.from_numpy(f), Ks, RTs, 24, 40)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.rasterize_mesh((torch.from_numpy(v), torch.from_numpy(f)), None, Ks, RTs, 24, 40)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.silhouette_stats(torch.zeros((1, 24, 40), dtype=torch.int32), torch.zeros((1, 24, 40), dtype=torch.uint8))
    with pytest.raises(pkg.GpnerfError, match="device tensor"):
        F.rasterize_mesh(v, f, Ks, RTs, 24, 40)              # host arrays go in as a pair with faces=None (uploaded), not as two tensors


def test_read_silhouette_metrics_on_hand_made_counts():
    F = importlib.import_module("gp-nerf_amd.frame")
    #          covered gt both either ignored
    counts = [[40, 50, 30, 60, 7],                           # iou 1/2, precision 3/4, recall 3/5
              [0, 0, 0, 0, 960],                             # everything ignored: 0 / 0 three times
              [0, 10, 0, 10, 0],                             # nothing drawn: precision 0 / 0
              [8, 0, 0, 8, 1]]                               # nothing to draw: recall 0 / 0
    r = F.read_silhouette_metrics(np.array(counts))
    assert r["per_view"]["iou"] == [0.5, 1.0, 0.0, 0.0]
    assert r["per_view"]["precision"] == [0.75, 1.0, 1.0, 0.0]
    assert r["per_view"]["recall"] == [0.6, 1.0, 0.0, 1.0]
    assert r["per_view"]["ignored"] == [7, 960, 0, 1]
    assert r["iou"] == 0.375 and r["precision"] == 0.6875 and r["recall"] == 0.65
    assert F.read_silhouette_metrics(torch.tensor(counts[:1]))["recall"] == 0.6


# ---- the restatement checks itself

def test_an_icospheres_silhouette_is_the_projected_disc():
    """a unit icosphere seen on the optical axis from distance d.  A sphere of radius r about the origin projects to a disc of radius
    R(r) = f r / sqrt(d^2 - r^2) pixels about the principal point.  The closed mesh lies inside the unit sphere and contains the
    sphere of radius rho = the least distance of a face's plane from the origin, so its silhouette lies between those two discs; a
    disc of radius R holds between pi (R - h)^2 and pi (R + h)^2 pixel centres, h = half a pixel's diagonal (every pixel whose
    centre is inside lies within R + h, every point within R - h lies in a pixel whose centre is inside); the snap moves a vertex by
    at most 1/512 pixel per axis, which 1/256 on h covers.  The covered area is therefore within [pi (R(rho) - h)^2, pi (R(1) + h)^2]."""
    v, f = mm.icosphere(3)
    H, W, d, focal = 70, 130, 64.0, 1600.0
    K = np.array([[focal, 0, 64.0], [0, focal, 34.0], [0, 0, 1]])
    RT = rc.look_at((d, 0, 0))
    cams = hull_cases.cams_of(K[None], RT[None])
    rc.assert_no_near_ties(v, f, cams)
    ref = rc.rasterize_np(v, f, cams, H, W)
    area = int(ref["stats"][0, 3])
    assert area == int((ref["face_id"] >= 0).sum()) and ref["stats"][0, 0] == len(f)
    tri = v.astype(np.float64)[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    rho = float(np.abs((n * tri[:, 0]).sum(axis=1) / np.linalg.norm(n, axis=1)).min())
    radius = lambda r: focal * r / np.sqrt(d * d - r * r)
    h = np.sqrt(2.0) / 2 + 1.0 / 256
    lo, hi = np.pi * (radius(rho) - h) ** 2, np.pi * (radius(1.0) + h) ** 2
    print(f"rho {rho:.5f}, disc radii {radius(rho):.3f} .. {radius(1.0):.3f} px, covered {area}, bounds [{lo:.1f}, {hi:.1f}]")
    assert 0.99 < rho < 1.0 and lo <= area <= hi
    # depth: the nearest point of the unit sphere is at d - 1; nothing of the mesh is farther than the centre
    depth = ref["depth"][0][ref["face_id"][0] >= 0]
    assert d - 1.0 - 1e-4 <= depth.min() <= d - rho + 1e-4 and depth.max() <= d


def test_two_triangles_sharing_an_edge_leave_no_hole_and_double_nothing():
    """faces 0 and 1 of `pixel_centres` share the hypotenuse x + y = 12, whose pixel centres (3, 9) .. (9, 3) both cover (edges are
    inclusive): together they cover the square [2, 10]^2 completely, every pixel once in face_id and in the statistics, and on the
    shared edge the nearer face -- at equal depth the smaller index -- wins"""
    c = rc.case("pixel_centres", "small", 1)
    fid = c["ref"]["face_id"][0]
    sq = fid[2:11, 2:11]
    assert ((sq == 0) | (sq == 1)).all(), "a hole on or beside the shared edge"
    only = rc.rasterize_np(c["v"], c["f"][:2], c["cams"], c["H"], c["W"])
    assert only["stats"][0].tolist() == [2, 0, 0, 81], "81 pixel centres in the square: the shared edge's are counted once"
    assert (only["face_id"][0] >= 0).sum() == 81
    each = [rc.rasterize_np(c["v"], c["f"][k:k + 1], c["cams"], c["H"], c["W"]) for k in (0, 1)]
    both = (each[0]["face_id"][0] >= 0) & (each[1]["face_id"][0] >= 0)
    assert sorted(zip(*np.nonzero(both))) == [(12 - x, x) for x in range(10, 1, -1)], "each face alone covers the shared edge's centres"
    for j, i in zip(*np.nonzero(both)):
        d0, d1 = each[0]["depth"][0, j, i], each[1]["depth"][0, j, i]
        assert only["face_id"][0, j, i] == (0 if d0 <= d1 else 1) and only["depth"][0, j, i] == min(d0, d1)
    # vertices on pixel centres are covered; the clockwise face 2 is drawn like the others; face 3 covers its three vertex pixels
    assert fid[2, 2] == 0 and fid[10, 10] == 1 and fid[3, 20] == 2 and fid[15, 24] == 2
    assert (fid == 3).sum() == 3 and fid[20, 30] == 3 and fid[20, 31] == 3 and fid[21, 30] == 3


def test_the_restatement_counts_skipped_faces_and_the_guard_band():
    c = rc.case("near_and_guard", "small", 1)
    assert c["ref"]["stats"][0, :3].tolist() == [2, 3, 0]     # faces 0 and 4 drawn; 1, 2, 3 skipped for a vertex
    d = rc.case("degenerate_mix", "small", 1)
    s = d["ref"]["stats"][0]
    assert s[1] == 4 and s[2] >= 1 and s[:3].sum() == len(d["f"])      # four bad faces; the face of three equal vertices has no area
    z = rc.case("zero_faces", "small", 3)
    assert not z["ref"]["stats"].any() and (z["ref"]["face_id"] == -1).all() and np.isposinf(z["ref"]["depth"]).all()
    t = rc.case("tie_cube", "small", 1)
    fid = t["ref"]["face_id"][0]
    assert (fid >= 0).any() and (fid < 12).all(), "of two coplanar copies the smaller index wins"
    masks = np.zeros((1,) + fid.shape, np.uint8)
    masks[0, :, 5:] = (fid[:, :-5] >= 0)
    masks[0, :3] = 100
    n = rc.silhouette_np(t["ref"]["face_id"], masks)[0]
    assert n[4] == 3 * fid.shape[1] and n[3] == n[0] + n[1] - n[2] and 0 < n[2] < n[0]
