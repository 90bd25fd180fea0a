"""CPU: the ray-casting restatements (tests/raycast_cases.py) against each other and against what the cases promise, the exact
antisymmetry of the edge function, THE WALK restated on a host grid against the brute force (and an exact walk without margins, which
loses hits), and the refusals of gpnerf_mesh_raycast, gpnerf_pixel_rays, the Python wrappers and MeshEvaluator(visible=True) -- none of
which needs a device."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import raycast_cases as rc

NAMES = [c["name"] for c in rc.cases()]


def case_of(name):
    return next(c for c in rc.cases() if c["name"] == name)


@pytest.mark.parametrize("name", NAMES)
def test_the_restatements_meet_what_the_cases_promise(name):
    case, ref = case_of(name), rc.reference(name)
    hit32, hit64 = np.isfinite(ref["t32"]), np.isfinite(ref["t64"])
    print(f"{name}: {len(case['rays'])} rays, {int(hit32.sum())} hit; | t32 - t64 | {rc.deviation(name):.3e}; hit / miss differs at "
          f"{int((hit32 != hit64).sum())}, the face at {int((ref['face32'] != ref['face64']).sum())} rays")
    assert np.array_equal(np.isnan(ref["t32"]), ~rc.ray_valid(case["rays"])) and np.array_equal(np.isnan(ref["t32"]), np.isnan(ref["t64"]))
    if case["hits"] is not None:
        promised = case["hits"] >= 0
        assert np.array_equal(hit32[promised], case["hits"][promised] == 1)
    if case["all_hit"]:
        assert hit32.all(), "the float32 restatement leaks"
    if case["interior"] is not None:
        # a condition on the INPUTS: rays aimed well inside a face (every weight >= 1/64) -- there float32 and float64 agree on hit /
        # miss and on the face, and the face is the one aimed at
        m = case["interior"]
        assert m.sum() >= 256 and hit32[m].all() and hit64[m].all() and np.array_equal(ref["face32"][m], ref["face64"][m])
        assert np.array_equal(ref["face32"][m], case["interior_face"])
        assert (ref["bary32"][m] >= 1.0 / 128).all() and (1 - ref["bary32"][m].sum(axis=1) >= 1.0 / 128).all()


def test_the_one_triangle_edge_cases():
    case, ref = case_of("one_triangle"), rc.reference("one_triangle")
    rays, t = case["rays"], ref["t32"]
    on_plane = np.flatnonzero((rays[:, 2] == 0) & (rays[:, 5] == 1) & (rays[:, 6] == 0))
    assert len(on_plane) == 1 and t[on_plane[0]] == 0                       # starts on the plane with tmin = 0: t = 0
    at_tmax = np.flatnonzero(rays[:, 7] == 1)
    assert len(at_tmax) == 1 and t[at_tmax[0]] == 1                         # t == tmax: a hit
    below = np.flatnonzero((rays[:, 7] < 1) & (rays[:, 7] > 0.99))
    assert len(below) == 1 and np.isinf(t[below[0]])                        # one ulp below: a miss
    assert ref["hits32"].max() == 1


def test_coincident_faces_the_lower_index_wins():
    case, ref = case_of("hygiene"), rc.reference("hygiene")
    f = case["faces"]
    # face 3 listed again (22) and face 5 under other vertex indices (23) give bit-equal t: the lower index wins.  Face 27 is face 5
    # with its vertices rotated: other roundings, so it is no tie and may win on its own t
    assert not {22, 23} & set(ref["face32"].tolist()), "bit-equal t: the lower index wins"
    assert {3, 5} <= set(ref["face32"].tolist())
    assert not {20, 21, 24, 25, 26} & set(ref["face32"].tolist()), "degenerate and invalid faces are never hit"
    assert len(f) == 28


def test_the_edge_function_is_exactly_antisymmetric():
    rng = np.random.default_rng(5)
    for scale in (1.0, 1e-20, 1e18):
        p = (rng.normal(size=(4, 200000)) * scale).astype(np.float32)
        p[:, ::7] = np.round(p[:, ::7] / scale * 4).astype(np.float32) * np.float32(scale / 4)     # many exact zeros among the results
        with np.errstate(over="ignore", invalid="ignore"):
            fwd, rev = rc.edge_function(p[0], p[1], p[2], p[3]), rc.edge_function(p[2], p[3], p[0], p[1])
        assert fwd.dtype == np.float32 and (fwd == 0).sum() > 100
        ok = ~np.isnan(fwd)
        assert np.array_equal(fwd[ok], -rev[ok])
        exact = p[0].astype(np.float64) * p[3].astype(np.float64) - p[1].astype(np.float64) * p[2].astype(np.float64)
        nz = ok & (fwd != 0) & np.isfinite(fwd)
        assert np.array_equal(np.sign(fwd[nz]), np.sign(exact[nz])), "a nonzero float32 sign is the exact sign"


GRIDS = {"one_triangle": (2, 2, 1), "shared_edge": (5, 5, 3), "fan": (4, 4, 2), "icosphere": (10, 10, 10), "cube": (4, 4, 4),
         "hygiene": (6, 6, 6), "flat": (9, 7, 1), "ray_hygiene": (4, 4, 4), "one_cell": (1, 1, 1), "axis_cap": (1024, 2, 1), "stress": (8, 8, 8)}


def test_the_walk_restated_finds_what_the_brute_force_finds_and_an_exact_walk_does_not():
    """THE WALK on a host grid, about 200 rays a case: the faces of the cells it visits give the brute force's t and face at every
    ray.  An exact Amanatides-Woo walk of the same grid -- no pads -- does not: rays aimed at a shared vertex graze cells the real
    ray never enters (the fan; this is what the pads are for)."""
    wrong, lost, cells = {}, {}, {}
    for case in rc.cases():
        name, ref = case["name"], rc.reference(case["name"])
        grid = rc.host_grid(case["vertices"], case["faces"], GRIDS[name])
        valid = np.flatnonzero(rc.ray_valid(case["rays"]))
        pick = valid[::max(1, len(valid) // 200)]
        wrong[name] = lost[name] = 0
        n_cells = [0, 0]
        for i in pick:
            for k, visited in enumerate((rc.walk_cells(case["rays"][i], grid), rc.dda_cells(case["rays"][i], grid))):
                t, face = rc.cast_through(case["rays"][i], case["vertices"], case["faces"], grid, visited)
                same = t.view(np.uint32) == ref["t32"][i].view(np.uint32) and face == ref["face32"][i]
                n_cells[k] += len(visited)
                if k == 0:
                    wrong[name] += not same
                else:
                    lost[name] += not same
        cells[name] = (n_cells[0] / len(pick), n_cells[1] / len(pick))
    print("cells per ray, THE WALK without its early stop / an exact walk:", {k: (round(a, 1), round(b, 1)) for k, (a, b) in cells.items()})
    print("rays an exact walk gets wrong:", lost)
    assert not any(wrong.values()), wrong
    assert lost["fan"] > 0


def test_pixel_rays_restated_hit_the_pixels_they_are_named_for():
    K, RT = rc.look_at([2.6, 1.1, 0.7], [0.05, -0.02, 0.03], 12, 20, 30.0)
    K[0, 1] = 0.25
    rays = rc.pixel_rays(K[None], RT[None], 12, 20, z_near=0.5)[0].astype(np.float64)
    p = rays[..., 0:3] + 2.5 * rays[..., 3:6]
    cam = p @ RT[:, :3].T + RT[:, 3]
    pix = cam @ K.T
    row, col = np.meshgrid(np.arange(12.0), np.arange(20.0), indexing="ij")
    assert np.abs(cam[..., 2] - 2.5).max() < 1e-5 and np.abs(pix[..., 0] / pix[..., 2] - col).max() < 1e-4 and np.abs(pix[..., 1] / pix[..., 2] - row).max() < 1e-4
    assert (rays[..., 6] == 0.5).all() and np.isinf(rays[..., 7]).all()


def test_raycast_refuses_bad_arguments_on_the_host(pkg):
    lib = pkg._lib.lib()
    P = 0x1000

    def call(rays=P, n=5, vertices=P, nv=3, faces=P, nf=1, grid=None, mode=0, t=P, face=P, bary=None):
        return lib.gpnerf_mesh_raycast(rays, n, vertices, nv, faces, nf, grid, mode, t, face, bary, None)

    assert call(n=0) == 0 and call(n=0, rays=None, t=None, face=None) == 0                  # a no-op
    for kw in (dict(n=-1), dict(nv=-1), dict(nf=0), dict(nf=1 << 31), dict(vertices=None), dict(faces=None), dict(mode=2), dict(mode=-1),
               dict(rays=None), dict(t=None), dict(face=None), dict(n=0, mode=7), dict(n=0, nf=0)):
        assert call(**kw) == -1, kw
    assert pkg._lib.RAYCAST_MODES == {"nearest": 0, "any": 1}
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(pkg.__file__), "..", "include", "gpnerf_hip.h")).read()
    assert "#define GPNERF_RAYCAST_NEAREST 0" in hdr and "#define GPNERF_RAYCAST_ANY 1" in hdr
    assert f"#define GPNERF_RAYCAST_MAX_VIEWS {pkg._lib.RAYCAST_MAX_VIEWS}" in hdr


def test_pixel_rays_refuses_bad_arguments_on_the_host(pkg):
    lib = pkg._lib.lib()
    K, RT = rc.look_at([2.0, 1.0, 0.5], [0, 0, 0], 8, 8, 10.0)
    good = np.concatenate([K.ravel(), RT.ravel()])

    def call(cams=good, n=1, H=8, W=8, z_near=1e-6, rays=0x1000):
        buf = None if cams is None else np.ascontiguousarray(np.tile(cams, max(n, 1)), np.float64)
        return lib.gpnerf_pixel_rays(None if buf is None else buf.ctypes.data_as(pkg._lib.DP), n, H, W, z_near, rays, None)

    flat_k, flat_r = good.copy(), good.copy()
    flat_k[8] = 0.0                                              # K's last row is zero: det 0
    flat_r[9 + 8:9 + 11] = flat_r[9 + 4:9 + 7]                   # two equal rows of R: det 0
    for kw in (dict(cams=None), dict(rays=None), dict(n=0), dict(n=9), dict(H=0), dict(W=16385), dict(z_near=0.0), dict(z_near=-1.0),
               dict(z_near=float("nan")), dict(z_near=float("inf")), dict(cams=flat_k), dict(cams=flat_r)):
        assert call(**kw) == -1, kw


def test_the_wrappers_refuse_cpu_tensors_and_bad_modes(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    v, f, r = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(4, 8)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.raycast_mesh(r, v, f)
    with pytest.raises(pkg.GpnerfError, match="'nearest' or 'any'"):
        F.raycast_mesh(r, v, f, mode="all")
    with pytest.raises(pkg.GpnerfError, match="MeshGrid"):
        F.raycast_mesh(r, grid=object())
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.mesh_visibility(torch.zeros(4, 3), [[1.0, 2.0, 3.0]], v, f)
    K, RT = rc.look_at([2.0, 1.0, 0.5], [0, 0, 0], 8, 8, 10.0)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.pixel_rays(K[None], RT[None], 8, 8, device="cpu")
    with pytest.raises(pkg.GpnerfError, match="cameras"):
        F.pixel_rays(np.tile(K, (9, 1, 1)), np.tile(RT, (9, 1, 1)), 8, 8)


def test_mesh_evaluator_visible_names_the_missing_key(pkg, tmp_path):
    ev = importlib.import_module("gp-nerf_amd.evaluator")
    e = ev.MeshEvaluator(str(tmp_path), 0.02, visible=True)
    assert e.visible and not ev.MeshEvaluator(str(tmp_path), 0.02).visible
    batch = {"frame_index": torch.tensor([0]), "gt_mesh": object(), "hull_masks": torch.zeros((1, 2, 8, 8), dtype=torch.uint8),
             "hull_Ks": torch.zeros((1, 2, 3, 3)), "hull_RTs": torch.zeros((1, 2, 3, 4))}
    with pytest.raises(pkg.GpnerfError, match=r"visible=True.*no 'axes'"):
        e._enqueue_visible({"mesh": object()}, batch)
    for key in ev.MeshEvaluator.SILHOUETTE_KEYS:
        with pytest.raises(pkg.GpnerfError, match=rf"visible=True.*'{key}'"):
            e._enqueue_visible({"mesh": object(), "axes": []}, {k: v for k, v in batch.items() if k != key})
    with pytest.raises(pkg.GpnerfError, match="hull_masks must be"):
        e._enqueue_visible({"mesh": object(), "axes": []}, dict(batch, hull_masks=torch.zeros((2, 8, 8), dtype=torch.uint8)))
    assert not e.has_mesh_metrics
