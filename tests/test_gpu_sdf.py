"""GPU: the truncated signed distance field (gpnerf_sdf.hip).  |sdf| and face_id are BIT-EQUAL to gpnerf_mesh_distance over the lattice
points with max_dist = band, in its grid and its brute-force form (both translation units compile csrc/gpnerf_tridist.h), and within
DESIGN 4.10's bound of the numpy restatement of include/gpnerf_hip.h (tests/sdf_cases.py); the band's edge, the signs against the
voxeliser's bits, determinism (two runs, a graph replay, a permutation of the faces), the statistics, the trilinear sampling bit-equal
to its float64 restatement, offset surfaces, and MeshEvaluator(signed=True) end to end.  Lattices of 12 x 10 x 9 to 40 x 40 x 33 points."""
import importlib
import os

import numpy as np
import pytest
import torch

import mesh_metric_cases as mm
import sdf_cases as sc
import voxelize_cases as vc

pytestmark = pytest.mark.gpu
F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
L = importlib.import_module("gp-nerf_amd._lib")
ev = importlib.import_module("gp-nerf_amd.evaluator")
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the cases' arrays are read-only)


def field(c, rule="case", want_face=True, faces=None):
    g = F.mesh_sdf(dev(c["v"]), dev(c["f"] if faces is None else faces), c["lo"], c["step"], c["dims"], c["band"],
                   rule=c["rule"] if rule == "case" else rule, want_face=want_face)
    torch.cuda.synchronize()
    return g


def host(g):
    return g.values.cpu().numpy(), (g.face.cpu().numpy() if g.face is not None else None), g.stats.cpu().numpy()


def bits_of(g):
    return vc.unpack_bits(g.voxels.bits.cpu().numpy().view(np.uint32), g.dims[2])


# ---- 1. bit equality with the list form, and the restatement within its bound

@pytest.mark.parametrize("name", sc.NAMES)
def test_the_field_is_bit_equal_to_point_mesh_distance(name):
    c = sc.case(name)
    g = field(c)
    values, face, stats = host(g)
    pts = dev(sc.lattice_points(c["lo"], c["step"], c["dims"]).reshape(-1, 3))
    tv, tf = dev(c["v"]), dev(c["f"])
    grid = F.build_mesh_grid(tv, tf)
    for form, res in (("grid", F.point_mesh_distance(pts, grid=grid, max_dist=c["band"])),
                      ("brute", F.point_mesh_distance(pts, tv, tf, max_dist=c["band"]))):
        d, f = res["dist"].cpu().numpy().reshape(c["dims"]), res["face"].cpu().numpy().reshape(c["dims"])
        want = np.where(np.isinf(d), np.float32(c["band"]), d)
        diff = np.abs(values).view(np.uint32) != want.view(np.uint32)
        print(f"{name} {form}: values that differ {int(diff.sum())} of {diff.size}, faces that differ {int((face != f).sum())}, "
              f"in band {int((f >= 0).sum())}")
        assert not np.isnan(d).any() and not diff.any() and np.array_equal(face, f), (name, form, np.argwhere(diff)[:5].tolist())
    ref = c["ref"]
    err = float(np.abs(np.abs(values).astype(np.float64) - ref["abs64"]).max())
    print(f"{name}: stats {stats.tolist()}, | field - float64 restatement | {err:.3e}, bound {c['bound']:.3e}, error / bound {err / c['bound']:.3f}")
    assert err <= c["bound"]
    if name == "twice":
        assert set(np.unique(face).tolist()) == {-1, 0}, "the same face twice: the lower index"
    if name == "tie_box":
        assert ref["tie"].sum() > 100 and np.array_equal(face[ref["tie"]], ref["face"][ref["tie"]]), "bit-equal distances: the lower index"
    if name == "beyond_band":
        assert stats[2] == 80 and (face < 80).all()
    if name == "quad_large":
        assert stats[3] == 2 and stats[0] == 2
    if name == "both_tiers":
        assert 0 < stats[3] < stats[0]


# ---- 2. the band's edge

def test_a_point_exactly_the_band_away_is_in():
    c = sc.case("plane")
    values, face, stats = host(field(c))
    assert c["band"] == 0.5 and (values[:, :, [2, 6]] == 0.5).all() and (face[:, :, [2, 6]] >= 0).all(), "z = +-0.5: the distance, and a face"
    assert (values[:, :, [0, 1, 7, 8]] == 0.5).all() and (face[:, :, [0, 1, 7, 8]] == -1).all(), "z = +-0.75 and beyond: the band, and none"
    assert np.array_equal(values, c["ref"]["abs"]) and np.array_equal(face, c["ref"]["face"]) and stats[4] == 12 * 10 * 5


# ---- 3. signs

@pytest.mark.parametrize("rule", ["parity", "nonzero"])
@pytest.mark.parametrize("name", ["box_nz9", "box_nz33", "box_nz64", "icosphere2"])
def test_the_sign_is_the_voxelisers_bit(name, rule):
    c = sc.case(name, want64=False)
    g = field(c, rule=rule, want_face=False)
    values, _, stats = host(g)
    occ = bits_of(g)
    assert g.face is None and occ.shape == c["dims"] and 0 < occ.sum() < occ.size
    assert np.array_equal(np.signbit(values), occ), np.argwhere(np.signbit(values) != occ)[:5].tolist()
    assert stats[5] == occ.sum() == int(g.voxels.occupied) and np.array_equal(np.abs(values), c["ref"]["abs"])
    given = F.mesh_sdf(dev(c["v"]), dev(c["f"]), c["lo"], c["step"], c["dims"], c["band"], voxels=g.voxels)
    assert given.voxels is g.voxels and given.values.cpu().numpy().tobytes() == values.tobytes()
    plain = field(c, rule=None, want_face=False)
    pv = plain.values.cpu().numpy()
    assert plain.voxels is None and not np.signbit(pv).any() and np.array_equal(pv, np.abs(values)) and plain.stats.cpu().numpy()[5] == 0
    with pytest.raises(L.GpnerfError, match="another lattice"):
        F.mesh_sdf(dev(c["v"]), dev(c["f"]), c["lo"] + 0.5, c["step"], c["dims"], c["band"], voxels=g.voxels)


# ---- 4. determinism

def test_two_runs_a_graph_replay_and_a_permutation_of_the_faces():
    cases = [sc.case(n) for n in ("both_tiers", "icosphere2")]
    tensors = [(dev(c["v"]), dev(c["f"])) for c in cases]

    def run():
        out = {}
        for i, (c, (tv, tf)) in enumerate(zip(cases, tensors)):
            g = F.mesh_sdf(tv, tf, c["lo"], c["step"], c["dims"], c["band"], rule=c["rule"], want_face=True)
            out[f"{i}_values"], out[f"{i}_face"], out[f"{i}_stats"] = g.values, g.face, g.stats
        return out

    first = {k: t.clone() for k, t in run().items()}          # (also loads the kernels before the capture)
    second = run()
    torch.cuda.synchronize()
    for k in first:
        assert first[k].cpu().numpy().tobytes() == second[k].cpu().numpy().tobytes(), k
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = run()
    for _ in range(2):
        for t in res.values():
            t.fill_(7)                                        # every output is written by the call; the workspace carries nothing over
        graph.replay()
        torch.cuda.synchronize()
        for k in first:
            assert first[k].cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes(), k
    rng = np.random.default_rng(3)
    for i, c in enumerate(cases):
        perm = rng.permutation(len(c["f"]))
        values, face, stats = host(field(c, faces=c["f"][perm]))
        assert values.tobytes() == first[f"{i}_values"].cpu().numpy().tobytes(), "the field does not depend on the order of the faces"
        was = first[f"{i}_face"].cpu().numpy()
        through = np.where(face >= 0, perm[np.maximum(face, 0)], -1)
        free = ~c["ref"]["tie"]
        print(f"case {i}: {int((~free).sum())} tied points, faces that differ elsewhere {int((through[free] != was[free]).sum())}")
        assert np.array_equal(through[free], was[free]) and np.array_equal(stats, first[f"{i}_stats"].cpu().numpy())


# ---- 5. stats

@pytest.mark.parametrize("name", sc.NAMES + ("guard",))
def test_the_stats_equal_the_restatements(name):
    c = sc.case(name)
    values, face, stats = host(field(c))
    ref = c["ref"]
    print(f"{name}: stats {dict(zip(sc.STATS, stats.tolist()))}")
    assert stats.dtype == np.int64 and np.array_equal(stats, ref["stats"]), (stats.tolist(), ref["stats"].tolist())
    assert stats[:3].sum() == len(c["f"]) and stats[4] == (face >= 0).sum() and stats[7] >= stats[4]
    assert np.array_equal(face, ref["face"]) and np.array_equal(values, ref["sdf"])      # (float32 on both sides, operation for operation)


# ---- 6. sample

def test_sample_is_bit_equal_to_the_float64_restatement():
    c = sc.case("icosphere2")
    g = field(c, want_face=False)
    values = g.values.cpu().numpy()
    rng = np.random.default_rng(12)
    dims = np.array(c["dims"])
    inside = c["lo"] + rng.uniform(0, dims - 1, (5000, 3)) * c["step"]
    around = c["lo"] + rng.uniform(-1, dims, (1000, 3)) * c["step"]
    odd = mm.f32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [0, 0, 1e38]])
    pts = mm.f32(np.concatenate([inside, around, odd]))
    got, want = g.sample(dev(pts)).cpu().numpy(), sc.sample_np(values, c["lo"], c["step"], pts)
    nan = np.isnan(want)
    print(f"sample: {len(pts)} points, {int(nan.sum())} outside, values that differ {int((got.view(np.uint32)[~nan] != want.view(np.uint32)[~nan]).sum())}")
    assert np.array_equal(np.isnan(got), nan) and nan[-len(odd):].all() and 100 < nan.sum() < 1000 and not nan[:5000].any()
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert g.sample(torch.zeros((0, 3), device=DEV)).shape == (0,)
    # a dyadic lattice: u is an integer at every lattice point, the last index (u == n - 1) included, and the stored value comes back
    t = sc.case("tie_box")
    gt = field(t, want_face=False)
    stored = gt.values.cpu().numpy()
    at = gt.sample(dev(sc.lattice_points(t["lo"], t["step"], t["dims"]).reshape(-1, 3))).cpu().numpy().reshape(t["dims"])
    assert np.array_equal(at, stored) and np.array_equal(at[-1, -1, -1], stored[-1, -1, -1]) and (stored < 0).any()
    hi = t["lo"] + (np.array(t["dims"]) - 1) * t["step"]
    edge = mm.f32([hi, hi + [1e-3, 0, 0], t["lo"], t["lo"] - [0, 1e-3, 0]])
    assert np.isnan(gt.sample(dev(edge)).cpu().numpy()).tolist() == [False, True, False, True]


# ---- 7. offset surfaces

def test_offset_meshes_lie_at_their_offset_and_beat_the_staircase():
    c = sc.case("offset_sphere", want64=False)
    assert c["step"].tolist() == [0.1] * 3 and c["band"] == 0.5
    g = field(c, want_face=False)
    tv, tf = dev(c["v"]), dev(c["f"])
    grid = F.build_mesh_grid(tv, tf)
    to_mesh = lambda p: F.point_mesh_distance(p, grid=grid)["dist"].cpu().numpy().astype(np.float64)
    for offset in (-0.2, 0.0, 0.2):
        v, f = g.offset_mesh(offset)
        # the float64 construction: the restated lattice values, the crossing of every sign-changing edge of sdf - offset by marching
        # cubes' linear formula, and the crossing's float64 distance to the mesh; e = 4 x its largest deviation from |offset|
        cross = sc.edge_crossings(c["ref"]["sdf"], c["lo"], c["step"], offset)
        e = 4.0 * float(np.abs(sc.nearest64(cross, c["v"], c["f"], c["band"]) - abs(offset)).max())
        dist = to_mesh(v)
        worst = float(np.abs(dist - abs(offset)).max())
        topo = F.read_mesh_topology(F.mesh_topology(f, int(v.shape[0])))
        print(f"offset {offset:+.1f}: {v.shape[0]} vertices ({len(cross)} restated crossings), {f.shape[0]} faces, | distance - |offset| | "
              f"{worst:.5f}, e {e:.5f}, watertight {topo['watertight']}")
        assert len(cross) == v.shape[0] and worst <= e and topo["watertight"] and topo["euler"] == 2
        if offset == 0.0:
            sv, sf = F.marching_cubes(g.voxels.dense(), 0.5)
            stairs = to_mesh((torch.from_numpy(c["lo"]).to(DEV) + sv.to(torch.float64) * torch.from_numpy(c["step"]).to(DEV)).to(torch.float32))
            print(f"offset 0: mean vertex distance to the mesh {dist.mean():.5f}, of the 0 / 1 cube's mesh {stairs.mean():.5f}")
            assert sf.shape[0] == f.shape[0] and dist.mean() < stairs.mean()
    with pytest.raises(L.GpnerfError, match="band"):
        g.offset_mesh(0.5)


# ---- 8. MeshEvaluator(signed=True)

PAD = ev.MeshEvaluator.PAD
AXES = [np.linspace(-0.6, 0.6, 13).astype(np.float32), np.linspace(-0.5, 0.7, 13).astype(np.float32), np.linspace(-0.6, 0.6, 13).astype(np.float32)]


def _sphere_frames(scale):
    """per frame: a geometry-mode output whose mesh is the scan's sphere scaled by `scale` about its centre, in index units of the
    padded 33^3 cube, and a batch whose gt_mesh is the sphere (radius 4 steps) in the axes' frame"""
    out = []
    for i in range(2):
        centre = np.array([PAD + 6.2, PAD + 5.7 + 0.5 * i, PAD + 6.4])
        pred = M.Mesh(*vc.placed_sphere(2, 4.0 * scale, centre))
        scan = M.Mesh(*vc.placed_sphere(2, 4.0, centre))
        output = {"cube": np.pad(np.zeros((13, 13, 13), np.float32), PAD), "mesh": pred, "axes": AXES}
        out.append((output, {"frame_index": torch.tensor([i]), "gt_mesh": scan.to_lattice_frame(AXES, PAD)}))
    return out


def test_mesh_evaluator_signed_end_to_end(tmp_path):
    got = {}
    for scale in (1.1, 0.9):
        e = ev.MeshEvaluator(str(tmp_path / str(scale)), 0.02, metric_samples=2000, signed=True, signed_band=8)
        for output, batch in _sphere_frames(scale):
            e.evaluate(output, batch)
        assert e.has_mesh_metrics
        got[scale] = e.summarize()
        assert e.summarize() == {} and not e.has_mesh_metrics     # reset
    grown, shrunk = got[1.1], got[0.9]
    print(f"signed: grown {grown['signed_mean']:.5f} (inside {grown['inside_fraction']}), shrunk {shrunk['signed_mean']:.5f} "
          f"(inside {shrunk['inside_fraction']}); one step is 0.1")
    assert grown["signed_mean"] > 0 > shrunk["signed_mean"] and grown["inside_fraction"] == 0.0 and shrunk["inside_fraction"] == 1.0
    # the spheres are 0.4 steps apart (0.04); the facets' sag (1.7 % of a radius of 0.44: 0.0075) and the trilinear interpolant of a
    # field of curvature 1 / 0.4 on a step of 0.1 (0.1^2 / (8 x 0.4): 0.003) move a sample's value by 0.0105 at most
    assert 0.0295 < grown["signed_mean"] < 0.0505 and -0.0505 < shrunk["signed_mean"] < -0.0295
    assert grown["signed_outside_lattice"] == 0 and grown["per_frame"]["signed_frame_index"] == [0, 1] and "chamfer" in grown
    table = np.load(tmp_path / "1.1" / "signed_metrics.npy")
    assert len(table) == 2 and table["samples"].tolist() == [2000, 2000] and table["signed_mean"].tolist() == grown["per_frame"]["signed_mean"]
    assert sorted(os.listdir(tmp_path / "1.1")) == ["mesh_metrics.npy", "pts", "signed_metrics.npy"]


def test_signed_off_changes_nothing_and_on_without_axes_raises(tmp_path):
    output, batch = _sphere_frames(1.1)[0]
    both = [ev.MeshEvaluator(str(tmp_path / name), 0.02, metric_samples=2000, signed=flag) for name, flag in (("plain", False), ("signed", True))]
    for m in both:
        m.evaluate(output, batch)
    plain, signed = (m.summarize() for m in both)
    is_new = lambda k: "signed" in k or k == "inside_fraction"
    assert not any(is_new(k) for k in plain) and not any(is_new(k) for k in plain["per_frame"])
    assert sorted(os.listdir(tmp_path / "plain")) == ["mesh_metrics.npy", "pts"]
    assert {k: v for k, v in signed.items() if not is_new(k) and k != "per_frame"} == {k: v for k, v in plain.items() if k != "per_frame"}
    assert {k: v for k, v in signed["per_frame"].items() if not is_new(k)} == plain["per_frame"]
    assert np.load(tmp_path / "plain" / "mesh_metrics.npy").tobytes() == np.load(tmp_path / "signed" / "mesh_metrics.npy").tobytes()
    on = ev.MeshEvaluator(str(tmp_path / "on"), 0.02, metric_samples=2000, signed=True)
    pts = torch.from_numpy(np.stack(np.meshgrid(*AXES, indexing="ij"), axis=-1))[None]
    with pytest.raises(L.GpnerfError, match="axes"):
        on.evaluate({"cube": output["cube"], "mesh": output["mesh"]}, dict(batch, pts=pts))
    off = ev.MeshEvaluator(str(tmp_path / "none"), 0.02, signed=True)
    off.evaluate(output, {"frame_index": batch["frame_index"]})     # no gt_mesh: nothing is enqueued
    assert not off.has_mesh_metrics and off.summarize() == {}
