"""CPU: the view-texturing restatement (tests/texture_cases.py) against what the definition promises -- the pixel convention on an
affine image, the sphere's counts, BEST's tie rule, the exact camera's frame and near plane -- and the refusals and workspace formula
of gpnerf_texture_points and its Python wrappers, none of which needs a device."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

import raycast_cases as rc
import texture_cases as tc


def test_an_affine_image_returns_the_affine_function_of_the_projection():
    """Channels affine in (column, row): bilinear interpolation reproduces an affine function, so the sample at an inside point IS that
    function of the float64 projection.  A half-pixel shift of the convention would show as half the slope (0.5 * 3 = 1.5 here)."""
    H, W = 17, 23
    coeffs = [(3.0, 0.0, 1.0), (0.0, -2.0, 50.0), (1.5, 0.25, -4.0)]
    image = tc.affine_image(H, W, coeffs).astype(np.float32)                  # small integers and quarters: exact in float32
    K, RT = rc.look_at([2.0, -1.5, 1.0], [0.1, 0.0, -0.1], H, W, 14.0)
    rng = np.random.default_rng(3)
    pts = (rng.normal(size=(4000, 3)) * 0.5).astype(np.float32)
    ref = tc.restate(pts, K[None], RT[None], image[None], sharpness=0)
    inside = ref["fate"][:, 0] == tc.USED
    assert inside.sum() > 1000
    x, y, _ = tc.project(pts[inside], K, RT)
    want = np.stack([a * x + b * y + c for a, b, c in coeffs], axis=1)
    got = tc.bilinear(image, x, y)                                             # float64, before the rounding to float32
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"affine image: {int(inside.sum())} inside points, | sample - affine | / max |affine| = {rel:.3e} (float64 rounding)")
    assert rel < 1e-9
    assert np.array_equal(ref["color"][inside], got.astype(np.float32))
    assert np.abs(ref["color"][inside] - want).max() < 1e-4 < 0.5 * 1.5


def test_the_sphere_counts():
    s = tc.sphere_case()
    v, f = s["vertices"], s["faces"]
    assert len(v) == 642 and len(f) == 1280
    images = np.zeros((6, 48, 48, 1), np.float32)
    free = tc.restate(v, s["Ks"], s["RTs"], images, normals=None)
    assert (free["fate"] == tc.USED).all(), "every vertex projects inside every image"
    ref = tc.restate(v, s["Ks"], s["RTs"], images, normals=s["normals"], cos_min=s["cos_min"], vertices=v, faces=f)
    facing = (ref["fate"] != tc.BACKFACING).sum(axis=0)
    assert facing.tolist() == [161] * 6, facing
    per_vertex = (ref["fate"] == tc.USED).sum(axis=1)
    assert per_vertex.min() >= 1 and per_vertex.max() <= 3
    reach = rc.ray_valid(ref["rows"].reshape(-1, 8))
    assert reach.sum() == 966
    assert (ref["fate"] == tc.OCCLUDED).sum() == 0, "the float32 restated intersection occludes none of the facing vertices"
    assert ref["stats"][:, tc.USED].tolist() == [161] * 6 and ref["stats"][:, tc.BACKFACING].tolist() == [481] * 6
    assert ref["totals"].tolist() == [642, 0]


def test_best_picks_the_lower_index_on_a_tie():
    """two mirror-image views (eyes at +x and -x of a point on the mirror plane, its normal in the plane): bit-equal weights"""
    H = W = 9
    K0, RT0 = rc.look_at([2.0, 0, 0], [0, 0, 0], H, W, 6.0)
    K1, RT1 = rc.look_at([-2.0, 0, 0], [0, 0, 0], H, W, 6.0)
    pts = np.array([[0, 0.25, 0.125], [0, -0.5, 0.25]], np.float32)
    nrm = np.array([[0, 1, 0], [0, 0, 1]], np.float32)
    # facing needs a > 0: n . (e - p) with n in the mirror plane: the same in both views
    nrm = -np.sign((nrm * pts).sum(axis=1, keepdims=True)) * nrm
    images = np.stack([np.full((H, W, 1), 0.25, np.float32), np.full((H, W, 1), 0.75, np.float32)])
    for Ks, RTs, first in ((np.stack([K0, K1]), np.stack([RT0, RT1]), 0.25), (np.stack([K1, K0]), np.stack([RT1, RT0]), 0.25)):
        ref = tc.restate(pts, Ks, RTs, images, normals=nrm, cos_min=0.0, mode="best", sharpness=1)
        assert (ref["fate"] == tc.USED).all()
        assert np.array_equal(ref["w"][:, 0], ref["w"][:, 1]) and (ref["w"] > 0).all(), "a mirror pair: bit-equal weights"
        assert ref["views"].tolist() == [1, 1] and ref["color"][:, 0].tolist() == [first, first]
    blend = tc.restate(pts, np.stack([K0, K1]), np.stack([RT0, RT1]), images, normals=nrm, cos_min=0.0, sharpness=1)
    assert blend["views"].tolist() == [3, 3] and blend["color"][:, 0].tolist() == [0.5, 0.5]


def test_the_exact_camera_frame_and_near_plane():
    e = tc.exact_case()
    images = tc.random_images(1, e["H"], e["W"], 3, 4)
    ref = tc.restate(e["points"], e["Ks"], e["RTs"], images, z_near=e["z_near"], sharpness=0)
    assert np.array_equal(ref["fate"][:, 0], e["expect"])
    assert ref["xy"][3:11, 0].tolist() == [[0, 4], [8, 4], [4, 0], [4, 8], [0, 0], [8, 0], [0, 8], [8, 8]]
    assert np.array_equal(ref["color"][10], images[0, 8, 8]) and np.array_equal(ref["color"][7], images[0, 0, 0])   # a corner is its pixel
    g = tc.general_case()
    full = tc.restate(g["points"], g["Ks"], g["RTs"], g["images"], normals=g["normals"], masks=g["masks"], vertices=g["vertices"],
                      faces=g["faces"], z_near=g["z_near"], fallback=g["fallback"])
    seen = {tc.FATES[k] for k in np.unique(full["fate"])}
    assert seen == set(tc.FATES), f"the general case reaches every fate, got {sorted(seen)}"
    assert (full["stats"].sum(axis=1) == len(g["points"])).all() and full["totals"].sum() == len(g["points"])
    assert full["totals"][1] > 0 and np.array_equal(full["color"][full["views"] == 0], g["fallback"][full["views"] == 0])


def test_the_workspace_formula(pkg):
    lib = pkg._lib.lib()
    a256 = lambda b: (b + 255) // 256 * 256
    formula = lambda n, v: a256(32 * n * v) + 2 * a256(4 * n * v) + a256(8 * n * v) + a256(n * v)
    for n, v in ((1, 1), (63, 3), (64, 8), (65, 8), (642, 6), (13000, 3), ((1 << 31) - 1, 8), (0, 1)):
        assert lib.gpnerf_texture_workspace_bytes(n, v) == formula(n, v), (n, v)
    assert lib.gpnerf_texture_workspace_bytes(1, 1) == 1280 and lib.gpnerf_texture_workspace_bytes(642, 6) == 189696
    for n, v in ((-1, 1), (1 << 31, 1), (5, 0), (5, 9)):
        assert lib.gpnerf_texture_workspace_bytes(n, v) == 0, (n, v)


def test_texture_points_refuses_bad_arguments_on_the_host(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    P = 0x1000
    K, RT = rc.look_at([2.0, 1.0, 0.5], [0, 0, 0], 8, 8, 10.0)
    cams = np.ascontiguousarray(np.tile(np.concatenate([K.ravel(), RT.ravel()]), 8), np.float64)
    bg = (C.c_float * 4)(0, 0, 0, 0)

    def call(points=P, n=5, normals=None, cams=cams, views=2, images=P, H=8, W=8, ch=3, masks=None, vertices=None, nv=0, faces=None, nf=0,
             grid=None, z_near=1e-6, cos_min=0.2, k=2, eps=1e-4, mode=0, fallback=None, bg=bg, ws=P, ws_bytes=None, color=P):
        need = lib.gpnerf_texture_workspace_bytes(max(min(n, 1 << 20), 0), min(max(views, 1), 8))
        return lib.gpnerf_texture_points(points, n, normals, None if cams is None else cams.ctypes.data_as(L.DP), views, images, H, W, ch, masks,
                                         vertices, nv, faces, nf, grid, z_near, cos_min, k, eps, mode, fallback, bg, ws,
                                         need if ws_bytes is None else ws_bytes, color, None, None, None, None, None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(points=None), dict(n=-1), dict(n=1 << 31), dict(cams=None), dict(views=0), dict(views=9), dict(images=None), dict(H=0),
               dict(W=0), dict(H=16385), dict(W=16385), dict(ch=0), dict(ch=5), dict(ch=4, images=P + 4), dict(z_near=0.0), dict(z_near=-1.0),
               dict(z_near=nan), dict(z_near=inf), dict(cos_min=-0.1), dict(cos_min=1.0), dict(cos_min=nan), dict(k=-1), dict(k=5),
               dict(eps=-1e-3), dict(eps=1.5), dict(eps=nan), dict(mode=2), dict(mode=-1), dict(nf=-1), dict(nf=1 << 31, vertices=P, faces=P),
               dict(nf=4, vertices=None, faces=P), dict(nf=4, vertices=P, faces=None), dict(nf=4, vertices=P, faces=P, nv=-1),
               dict(nf=0, grid=P), dict(bg=None), dict(ws=None), dict(ws=P + 8), dict(ws_bytes=1024)):
        assert call(**kw) == -1, kw
    assert L.TEXTURE_MODES == {"blend": 0, "best": 1}
    hdr = open(os.path.join(os.path.dirname(pkg.__file__), "..", "include", "gpnerf_hip.h")).read()
    for i, name in enumerate(L.TEXTURE_STATS):
        assert f"#define GPNERF_TEXTURE_{name.upper()} {i}\n" in hdr, name
        assert getattr(L, f"TEXTURE_{name.upper()}") == i and tc.FATES[i] == name
    assert f"#define GPNERF_TEXTURE_FATES {L.TEXTURE_FATES}\n" in hdr and L.TEXTURE_FATES == len(L.TEXTURE_STATS)
    assert "#define GPNERF_TEXTURE_BLEND 0\n" in hdr and "#define GPNERF_TEXTURE_BEST 1\n" in hdr
    assert f"#define GPNERF_TEXTURE_MAX_VIEWS {L.TEXTURE_MAX_VIEWS}\n" in hdr and f"#define GPNERF_TEXTURE_MAX_SHARPNESS {L.TEXTURE_MAX_SHARPNESS}\n" in hdr


def test_the_wrappers_refuse_cpu_tensors_and_bad_options(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    K, RT = rc.look_at([2.0, 1.0, 0.5], [0, 0, 0], 8, 8, 10.0)
    pts, img = torch.zeros(4, 3), torch.zeros(1, 8, 8, 3)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.texture_points(pts, K[None], RT[None], img)
    with pytest.raises(pkg.GpnerfError, match="'blend' or 'best'"):
        F.texture_points(pts, K[None], RT[None], img, mode="mean")
    with pytest.raises(pkg.GpnerfError, match="want names"):
        F.texture_points(pts, K[None], RT[None], img, want=("colour",))
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.texture_mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), K[None], RT[None], img)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.face_vertex_normals(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))


def test_read_texture_stats_names_and_fractions(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    stats = np.array([[6, 1, 1, 0, 2, 0], [0, 0, 0, 0, 10, 0]], np.int64)
    r = F.read_texture_stats(stats, np.array([6, 4], np.int64))
    assert r["per_view"]["used"] == [6, 0] and r["per_view"]["backfacing"] == [2, 10] and set(r["per_view"]) == set(pkg._lib.TEXTURE_STATS)
    assert r["used_fraction"] == [0.6, 0.0] and (r["seen"], r["unseen"], r["seen_fraction"]) == (6, 4, 0.6)
    assert F.read_texture_stats(np.zeros((1, 6)), np.zeros(2))["seen_fraction"] == 0.0
