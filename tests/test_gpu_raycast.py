"""GPU: casting rays against a mesh (gpnerf_raycast.hip).  t, face and bary of the walk through the grid are BIT-EQUAL to the brute-force
form's at every ray of every case of tests/raycast_cases.py, and both to the numpy float32 restatement of include/gpnerf_hip.h's THE
INTERSECTION; determinism (a graph capture and two replays, a permutation of the faces); ANY mode; an overflowed grid; the accuracy
against the float64 restatement; gpnerf_pixel_rays bit-equal to its restatement; the rays against the rasteriser; mesh_visibility on
a sphere; MeshEvaluator(visible=True) end to end.  At most 4 096 rays and 1 280 faces per case."""
import importlib

import numpy as np
import pytest
import torch

import mesh_metric_cases as mm
import raycast_cases as rc
import voxelize_cases as vc

pytestmark = pytest.mark.gpu
F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
L = importlib.import_module("gp-nerf_amd._lib")
ev = importlib.import_module("gp-nerf_amd.evaluator")
DEV = "cuda:0"
NAMES = [c["name"] for c in rc.cases()]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the cases' arrays are shared)


def case_of(name):
    return next(c for c in rc.cases() if c["name"] == name)


def host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def cast(case, form, mode="nearest", rays=None, faces=None, want_bary=True):
    v, f = dev(case["vertices"]), dev(case["faces"] if faces is None else faces)
    r = dev(case["rays"] if rays is None else rays)
    if form == "grid":
        return host(F.raycast_mesh(r, grid=F.build_mesh_grid(v, f, cell_cap=case["cell_cap"]), mode=mode, want_bary=want_bary))
    return host(F.raycast_mesh(r, v, f, mode=mode, want_bary=want_bary))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- 1. bit equality: grid == brute == the float32 restatement

@pytest.mark.parametrize("name", NAMES)
def test_grid_brute_and_restatement_agree_bit_for_bit(name):
    case, ref = case_of(name), rc.reference(name)
    brute, grid = cast(case, "brute"), cast(case, "grid")
    hit = np.isfinite(ref["t32"])
    print(f"{name}: {len(case['rays'])} rays, {len(case['faces'])} faces, {int(hit.sum())} hit, {int(np.isnan(ref['t32']).sum())} not rays")
    for form, got in (("brute", brute), ("grid", grid)):
        wrong = np.flatnonzero(got["t"].view(np.uint32) != ref["t32"].view(np.uint32))
        assert not len(wrong), (name, form, wrong[:5].tolist(), got["t"][wrong[:5]].tolist(), ref["t32"][wrong[:5]].tolist())
        assert np.array_equal(got["face"], ref["face32"]), (name, form, np.flatnonzero(got["face"] != ref["face32"])[:5].tolist())
        assert same_bits(got["bary"][hit], ref["bary32"][hit]) and np.isnan(got["bary"][~hit]).all(), (name, form)
    assert same_bits(grid["t"], brute["t"]) and np.array_equal(grid["face"], brute["face"]) and same_bits(grid["bary"][hit], brute["bary"][hit])
    if case["all_hit"]:
        assert hit.all() and (grid["face"] >= 0).all(), "a ray leaked between faces that share an edge or a vertex"
    if case["hits"] is not None:
        promised = case["hits"] >= 0
        assert np.array_equal(np.isfinite(grid["t"])[promised], case["hits"][promised] == 1)
    if name == "ray_hygiene":
        n_bad = case["n_bad"]
        assert np.isnan(grid["t"][:n_bad]).all() and (grid["face"][:n_bad] == -1).all() and not np.isnan(grid["t"][n_bad:]).any()


def test_the_forced_grids_are_what_their_cases_say():
    shapes = {}
    for name in ("one_cell", "axis_cap", "flat", "cube"):
        case = case_of(name)
        shapes[name] = F.build_mesh_grid(dev(case["vertices"]), dev(case["faces"]), cell_cap=case["cell_cap"]).header()["cells"]
    print(shapes)
    assert shapes["one_cell"] == [1, 1, 1] and shapes["axis_cap"][0] == 1024 and shapes["axis_cap"][2] == 1
    assert shapes["flat"][2] == 1 and shapes["cube"] == [4, 4, 4]


def test_ray_counts_around_a_wavefront_and_without_bary():
    case, ref = case_of("icosphere"), rc.reference("icosphere")
    for n in (1, 63, 64, 65):
        for form in ("brute", "grid"):
            got = cast(case, form, rays=case["rays"][:n], want_bary=False)
            assert "bary" not in got and same_bits(got["t"], ref["t32"][:n]) and np.array_equal(got["face"], ref["face32"][:n]), (n, form)
    v, f = dev(case["vertices"]), dev(case["faces"])
    none = F.raycast_mesh(torch.empty((0, 8), device=DEV), v, f)
    assert none["t"].shape == (0,) and none["face"].shape == (0,)
    shaped = F.raycast_mesh(dev(case["rays"][:24].reshape(2, 3, 4, 8)), v, f, want_bary=True)
    assert shaped["t"].shape == (2, 3, 4) and shaped["bary"].shape == (2, 3, 4, 2)


# ---- 2. determinism

def test_graph_replay_and_face_permutation():
    case, ref = case_of("icosphere"), rc.reference("icosphere")
    v, f, r = dev(case["vertices"]), dev(case["faces"]), dev(case["rays"])
    grid = F.build_mesh_grid(v, f)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = F.raycast_mesh(r, grid=grid, want_bary=True)
    for _ in range(2):
        for t in res.values():
            t.fill_(7)
        g.replay()
        got = host(res)
        assert same_bits(got["t"], ref["t32"]) and np.array_equal(got["face"], ref["face32"])
        assert got["bary"].tobytes() == cast(case, "grid")["bary"].tobytes()
    perm = np.random.default_rng(3).permutation(len(case["faces"]))
    shuffled = np.ascontiguousarray(case["faces"][perm])
    want_t, want_face, _, _ = rc.closest_hit(case["rays"], case["vertices"], shuffled)
    for form in ("brute", "grid"):
        got = cast(case, form, faces=shuffled)
        assert same_bits(got["t"], ref["t32"]), "the minimum does not depend on the order of the faces"
        assert np.array_equal(got["face"], want_face)
        back = np.where(got["face"] >= 0, perm[np.maximum(got["face"], 0)], -1)
        ties = np.where(want_face >= 0, perm[np.maximum(want_face, 0)], -1) != ref["face32"]      # the restatement's own: equal t, another index
        assert np.array_equal(back[~ties], ref["face32"][~ties])
        print(f"permuted faces, {form}: {int(ties.sum())} rays whose winner is a tie")


# ---- 3. ANY mode, an overflowed grid

@pytest.mark.parametrize("name", ["icosphere", "cube", "hygiene", "axis_cap", "ray_hygiene", "stress"])
def test_any_mode_is_occluded_iff_nearest_hits(name):
    case, ref = case_of(name), rc.reference(name)
    hit, bad = np.isfinite(ref["t32"]), np.isnan(ref["t32"])
    for form in ("brute", "grid"):
        got = cast(case, form, mode="any")
        assert np.array_equal(got["t"][~bad] == 0, hit[~bad]) and np.isinf(got["t"][~bad & ~hit]).all() and np.isnan(got["t"][bad]).all(), (name, form)
        assert np.array_equal(got["face"] >= 0, hit) and np.isnan(got["bary"]).all()
        if form == "brute":                                     # the lowest index among the accepted faces
            v, f = case["vertices"], case["faces"].astype(np.int64)
            ok = mm.valid_faces(v, f)
            rows = np.flatnonzero(hit)[:256]
            acc = rc.intersect(case["rays"][rows], v[f[ok][:, 0]], v[f[ok][:, 1]], v[f[ok][:, 2]])[0]
            assert np.array_equal(got["face"][rows], np.flatnonzero(ok)[acc.argmax(axis=1)])


def test_an_overflowed_grid_answers_nan():
    case = case_of("icosphere")
    v, f, r = dev(case["vertices"]), dev(case["faces"]), dev(case["rays"][:300])
    grid = F.build_mesh_grid(v, f, entry_cap=8, check=False)
    assert grid.header()["status"] == L.GRID_OVERFLOW
    before = grid.workspace.clone()
    for mode in ("nearest", "any"):
        got = host(F.raycast_mesh(r, grid=grid, mode=mode, want_bary=True))
        assert np.isnan(got["t"]).all() and (got["face"] == -1).all() and np.isnan(got["bary"]).all()
    assert torch.equal(before, grid.workspace), "a grid that is not OK is neither read nor written"


# ---- 4. accuracy against float64

@pytest.mark.parametrize("name", NAMES)
def test_accuracy_against_the_float64_restatement(name):
    """the bound is 4 x the float32 RESTATEMENT's own deviation from the float64 one (at least one ulp of the largest t), over the
    rays both restatements hit"""
    case, ref = case_of(name), rc.reference(name)
    got = cast(case, "grid")
    both = np.isfinite(ref["t32"]) & np.isfinite(ref["t64"])
    if not both.any():
        return
    dev32 = rc.deviation(name)
    bound = max(4.0 * dev32, float(np.spacing(np.float32(np.abs(ref["t64"][both]).max()))))
    err = float(np.abs(got["t"][both].astype(np.float64) - ref["t64"][both]).max())
    print(f"{name}: | t - float64 restatement | {err:.3e}, the float32 restatement's own {dev32:.3e}, bound {bound:.3e}")
    assert err <= bound


# ---- 5. pixel rays, and the rays against the rasteriser

def _cameras(H, W):
    K0, RT0 = rc.look_at([2.6, 1.1, 0.7], [0.05, -0.02, 0.03], H, W, 1.1 * W)
    K1, RT1 = rc.look_at([-0.4, -3.1, 1.9], [0, 0, 0], H, W, 0.9 * W)
    K1[0, 1] = 0.37                                              # a skewed K: the general inverse
    return np.stack([K0, K1]), np.stack([RT0, RT1])


def test_pixel_rays_are_bit_equal_to_their_restatement():
    Ks, RTs = _cameras(48, 48)
    got = F.pixel_rays(Ks, RTs, 48, 48, z_near=0.125)
    torch.cuda.synchronize()
    want = rc.pixel_rays(Ks, RTs, 48, 48, z_near=0.125)
    assert got.shape == (2, 48, 48, 8) and got.cpu().numpy().tobytes() == want.tobytes()
    odd = F.pixel_rays(Ks[:1], RTs[:1], 5, 67).cpu().numpy()
    assert odd.tobytes() == rc.pixel_rays(Ks[:1], RTs[:1], 5, 67).tobytes()
    # t is camera depth: the camera-z component of every direction is 1
    d = want[0, :, :, 3:6].astype(np.float64) @ RTs[0][:, :3].T
    assert np.abs(d[..., 2] - 1).max() < 1e-6


def test_rays_agree_with_the_rasteriser():
    """Case 3's sphere in a 64 x 64 camera.  Coverage: at every pixel whose 3 x 3 neighbourhood in the raster's face-id map is all
    covered or all empty the ray's hit / miss equals it.  Depth where the two name the same face: the rasteriser snaps projected
    vertices to 1/256 of a pixel, i.e. moves each by at most 1/512 per axis, which moves the point at which the face's plane is
    evaluated by no more than that in pixels; the face's depth changes by at most (its vertices' depth spread / its smallest height
    in pixels) per pixel, so the bound per face is spread / height * 3/256 (x 2 for both axes and a margin), plus 4 x the float32
    restatement's deviation."""
    H = W = 64
    case = case_of("icosphere")
    v, f = dev(case["vertices"]), dev(case["faces"])
    Ks, RTs = _cameras(H, W)
    Ks, RTs = Ks[:1], RTs[:1]
    drawn = host(F.rasterize_mesh(v, f, Ks, RTs, H, W))
    got = host(F.raycast_mesh(F.pixel_rays(Ks, RTs, H, W), grid=F.build_mesh_grid(v, f)))
    fid, depth, t, face = drawn["face_id"][0], drawn["depth"][0], got["t"][0], got["face"][0]
    covered = fid >= 0
    pad = np.pad(covered, 1, mode="edge")
    windows = np.stack([pad[i:i + H, j:j + W] for i in range(3) for j in range(3)])
    plain = windows.all(axis=0) | ~windows.any(axis=0)
    assert plain.sum() > 0.8 * H * W and covered.sum() > 500
    assert np.array_equal(np.isfinite(t)[plain], covered[plain])
    same = covered & (face == fid)
    print(f"rasteriser: {int(covered.sum())} covered pixels, another face at {float((covered & (face != fid)).sum() / covered.sum()):.4f} of them")
    cam = case["vertices"].astype(np.float64) @ RTs[0][:, :3].T + RTs[0][:, 3]
    pix = (cam @ Ks[0].T)[:, :2] / cam[:, 2:3]
    tri, z = pix[case["faces"]], cam[:, 2][case["faces"]]
    e = [tri[:, (k + 1) % 3] - tri[:, k] for k in range(3)]
    area2 = np.abs(e[0][:, 0] * e[1][:, 1] - e[0][:, 1] * e[1][:, 0])
    height = area2 / np.max([np.linalg.norm(x, axis=1) for x in e], axis=0)
    per_face = (z.max(axis=1) - z.min(axis=1)) / height * (3.0 / 256.0) + 4.0 * rc.deviation("icosphere")
    err = np.abs(t[same].astype(np.float64) - depth[same])
    print(f"rasteriser: | t - depth | max {err.max():.3e} over {int(same.sum())} pixels, the bound there {per_face[fid[same]][err.argmax()]:.3e}")
    assert (err <= per_face[fid[same]]).all()


# ---- 6. visibility

def test_mesh_visibility_on_a_sphere():
    """a vertex of the (convex) icosphere sees an eye outside iff its outward normal faces the eye; vertices with |cos| < 0.2 are
    left out.  The float32 restatement is held to the same rule first."""
    v, f = mm.icosphere(3)
    eyes = mm.f32([[4.0, 0.5, 0.25], [-1.0, -3.5, 2.0], [0.3, 0.2, -5.0]])
    to_eye = eyes[None].astype(np.float64) - v[:, None].astype(np.float64)
    cos = (v[:, None].astype(np.float64) * to_eye).sum(axis=2) / np.linalg.norm(to_eye, axis=2) / np.linalg.norm(v, axis=1)[:, None]
    use, facing = np.abs(cos) >= 0.2, cos > 0
    rows = np.concatenate([np.broadcast_to(v[:, None], to_eye.shape), (eyes[None] - v[:, None]).astype(np.float32),
                           np.full(to_eye.shape[:2] + (1,), 1e-4, np.float32), np.ones(to_eye.shape[:2] + (1,), np.float32)], axis=2).astype(np.float32)
    free = np.isinf(rc.closest_hit(rows.reshape(-1, 8), v, f)[0]).reshape(use.shape)
    assert np.array_equal(free[use], facing[use]) and use.sum() > 1200
    tv, tf = dev(v), dev(f)
    for kw in (dict(grid=F.build_mesh_grid(tv, tf)), dict(vertices=tv, faces=tf)):
        vis = F.mesh_visibility(tv, eyes, **kw)
        torch.cuda.synchronize()
        assert vis.dtype == torch.uint8 and tuple(vis.shape) == use.shape
        assert np.array_equal(vis.cpu().numpy().astype(bool), free)


# ---- 7. MeshEvaluator(visible=True)

PAD = ev.MeshEvaluator.PAD
AXES = [np.linspace(-0.6, 0.6, 13).astype(np.float32), np.linspace(-0.5, 0.7, 13).astype(np.float32), np.linspace(-0.6, 0.6, 13).astype(np.float32)]
HW = 40


def _visible_frame(scale, i=0):
    centre = np.array([PAD + 6.2, PAD + 5.7 + 0.5 * i, PAD + 6.4])
    pred, scan = M.Mesh(*vc.placed_sphere(2, 4.0 * scale, centre)), M.Mesh(*vc.placed_sphere(2, 4.0, centre))
    mid = [float(a[0]) + 0.1 * (c - PAD) for a, c in zip(AXES, centre)]
    cams = [rc.look_at(np.array(mid) + off, mid, HW, HW, 1.5 * HW) for off in ([2.0, 0.3, 0.2], [-0.2, -1.8, 0.9])]
    batch = {"frame_index": torch.tensor([i]), "gt_mesh": scan.to_lattice_frame(AXES, PAD), "hull_masks": torch.zeros((1, 2, HW, HW), dtype=torch.uint8),
             "hull_Ks": torch.from_numpy(np.stack([c[0] for c in cams]))[None], "hull_RTs": torch.from_numpy(np.stack([c[1] for c in cams]))[None]}
    return {"cube": np.pad(np.zeros((13, 13, 13), np.float32), PAD), "mesh": pred, "axes": AXES}, batch


def test_mesh_evaluator_visible_end_to_end(tmp_path):
    got = {}
    for scale in (1.0, 1.1):
        e = ev.MeshEvaluator(str(tmp_path / str(scale)), 0.02, metric_samples=2000, visible=True)
        for i in range(2):
            e.evaluate(*_visible_frame(scale, i))
        assert e.has_mesh_metrics
        got[scale] = e.summarize()
        assert e.summarize() == {} and not e.has_mesh_metrics
    same, grown = got[1.0], got[1.1]
    assert same["visible_depth_mean"] == 0.0 and same["visible_depth_max"] == 0.0 and same["visible_hit_disagreement"] == 0.0
    assert grown["visible_depth_mean"] > 0 and 0 < grown["visible_hit_disagreement"] < 0.5 and "chamfer" in grown
    assert grown["per_frame"]["visible_frame_index"] == [0, 1] and len(grown["per_frame"]["visible_depth_rms"]) == 2
    table = np.load(tmp_path / "1.1" / "visible_metrics.npy")
    assert table["frame_index"].tolist() == [0, 1] and (table["pixels_both"] + table["pixels_one"] + table["pixels_neither"] == 2 * HW * HW).all()
    # the float64 restatement's value for the same rays (frame 0): within 4 x the float32 restatement's deviation of it per pixel,
    # so the means agree to that too
    output, batch = _visible_frame(1.1, 0)
    rays = rc.pixel_rays(batch["hull_Ks"][0].numpy(), batch["hull_RTs"][0].numpy(), HW, HW).reshape(-1, 8)
    meshes = [output["mesh"].to_lattice_frame(AXES, PAD), batch["gt_mesh"]]
    t64 = [rc.closest_hit(rays, m.vertices, m.faces, np.float64)[0] for m in meshes]
    t32 = [rc.closest_hit(rays, m.vertices, m.faces, np.float32)[0] for m in meshes]
    both = np.isfinite(t64[0]) & np.isfinite(t64[1])
    assert np.array_equal(both, np.isfinite(t32[0]) & np.isfinite(t32[1]))
    own = max(float(np.abs(a[both].astype(np.float64) - b[both]).max()) for a, b in zip(t32, t64))
    want = float(np.abs(t64[0][both] - t64[1][both]).mean())
    print(f"visible_depth_mean {grown['per_frame']['visible_depth_mean'][0]:.6e}, float64 restatement {want:.6e}, bound {8 * own:.3e}")
    assert abs(grown["per_frame"]["visible_depth_mean"][0] - want) <= 8.0 * own
    assert table["pixels_both"][0] == int(both.sum())


def test_visible_off_changes_nothing_and_missing_keys_raise(tmp_path):
    output, batch = _visible_frame(1.1)
    plain = ev.MeshEvaluator(str(tmp_path / "plain"), 0.02, metric_samples=2000)
    plain.evaluate(output, batch)
    res = plain.summarize()
    assert not any("visible" in k for k in res) and not any("visible" in k for k in res["per_frame"])
    on = ev.MeshEvaluator(str(tmp_path / "on"), 0.02, metric_samples=2000, visible=True)
    pts = torch.from_numpy(np.stack(np.meshgrid(*AXES, indexing="ij"), axis=-1))[None]
    with pytest.raises(L.GpnerfError, match="axes"):
        on.evaluate({"cube": output["cube"], "mesh": output["mesh"]}, dict(batch, pts=pts))
    with pytest.raises(L.GpnerfError, match="hull_Ks"):
        on.evaluate(output, {k: v for k, v in batch.items() if k != "hull_Ks"})
    off = ev.MeshEvaluator(str(tmp_path / "none"), 0.02, visible=True)
    off.evaluate(output, {"frame_index": batch["frame_index"]})     # no gt_mesh: nothing is enqueued
    assert not off.has_mesh_metrics and off.summarize() == {}
