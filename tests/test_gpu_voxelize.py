"""GPU: the mesh voxeliser (gpnerf_voxelize.hip) against the numpy restatement of include/gpnerf_hip.h (tests/voxelize_cases.py): bits
and all six statistics EQUAL -- both sides evaluate the same unfused float64 expressions and exact int64 edge functions, and the cases
hold no crossing near a lattice index --, the round trip through the device's own marching cubes exact, two runs and a graph replay
identical, the packed-cube operations against numpy, and MeshEvaluator(volume=True) end to end.  Lattices of 12 x 10 x 9 to
40 x 40 x 20 points, 34^3 for the 108 k-face mesh, and 3 x 3 x 2100 for toggle rows of more than a wavefront's words."""
import importlib
import os

import numpy as np
import pytest
import torch

import mesh_metric_cases as mm
import voxelize_cases as vc

pytestmark = pytest.mark.gpu
F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
L = importlib.import_module("gp-nerf_amd._lib")
ev = importlib.import_module("gp-nerf_amd.evaluator")
DEV = "cuda:0"
RULES = ("parity", "nonzero")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the cases' arrays are read-only)


def words(grid):
    return grid.bits.cpu().numpy().view(np.uint32)


def voxelize(c, rule):
    grid = F.voxelize_mesh(dev(c["v"]), dev(c["f"]), c["lo"], c["step"], c["dims"], rule=rule)
    torch.cuda.synchronize()
    return grid


def assert_equal_to_restatement(what, grid, ref):
    got_bits, got_stats = words(grid), grid.stats.cpu().numpy()
    diff = got_bits != ref["bits"]
    print(f"{what}: stats {got_stats.tolist()} (restatement {ref['stats'].tolist()}), words that differ {int(diff.sum())} of {diff.size}")
    assert got_stats.dtype == np.int64 and np.array_equal(got_stats, ref["stats"]), what
    assert got_bits.shape == ref["bits"].shape and not diff.any(), (what, np.argwhere(diff)[:5].tolist())


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", vc.NAMES)
def test_bits_and_stats_equal_the_restatement(name, rule):
    c = vc.case(name, rule)
    grid = voxelize(c, rule)
    ref = c["ref"]
    assert_equal_to_restatement(f"{name} {rule}", grid, ref)
    nz = c["dims"][2]
    assert grid.dims == c["dims"] and grid.bits.shape[2] == (nz + 31) // 32
    assert int(grid.occupied) == ref["stats"][5]
    if name == "box_nz9":
        assert ref["stats"].tolist() == [4, 0, 8, 30, 0, 60]
    if name == "wide_large":                                  # (these two: every used face beyond the small tier, none of a square box)
        assert ref["stats"].tolist() == [4, 0, 8, 720, 0, 5040]
    if name == "wedge_large":
        assert ref["stats"].tolist() == [4, 0, 0, 610, 0, 1315]
    if name == "box_nz33":
        assert ref["occ"][2, 3, 32] and ref["bits"][2, 3, 1] == 1, "the second word's one bit is set"
    if name == "box_nz64":
        assert ref["occ"][2, 3, 63] and ref["occ"][8, 1, 63] and not ref["stats"][4], "crossings at kc = nz: the toggle row's extra word"
    if name in ("box_large", "both_tiers"):                  # (the case is what it says: faces beyond the small tier's 256 columns)
        assert ref["stats"][3] >= 1800
    if name == "both_tiers":
        assert ref["stats"][0] > 300, "and faces of the small tier beside them"
    if name == "all_cases":
        assert len(c["f"]) > 100000 and np.array_equal(ref["occ"], vc.field("all_cases") > vc.ISO)
    if name == "degenerate":
        assert ref["stats"][:3].tolist() == [4, 5, 10]
    if name == "twice":
        assert ref["stats"][5] == (0 if rule == "parity" else 60)
    if name == "two_boxes":
        assert ref["stats"][5] == (136 if rule == "parity" else 148)
    if name == "hemisphere":
        assert ref["stats"][4] > 0
    if name == "zero_faces":
        assert not ref["stats"].any() and not words(grid).any()
    if name == "tall":
        assert nz // 32 + 1 > 64 and ref["stats"][5] > 10000


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", vc.FIELDS)
def test_the_round_trip_on_the_device_is_exact(name, rule):
    """voxelize_mesh(*marching_cubes(cube)) == voxelize_cube(cube, iso), bit for bit, with nothing from numpy in between"""
    f = vc.field(name)
    cube = dev(f)
    v, faces = F.marching_cubes(cube, float(vc.ISO))
    grid = F.voxelize_mesh(v, faces, (0, 0, 0), (1, 1, 1), f.shape, rule=rule)
    direct = F.voxelize_cube(cube, float(vc.ISO))
    inside = f > vc.ISO
    got, want = words(grid), words(direct)
    stats = grid.stats.cpu().numpy()
    print(f"{name} {rule}: {faces.shape[0]} faces, stats {stats.tolist()}, words that differ {int((got != want).sum())}")
    assert np.array_equal(want, vc.pack_bits(inside)), "voxelize_cube is cube > iso, packed"
    assert np.array_equal(got, want)
    assert stats[5] == inside.sum() and stats[4] == 0 and stats[1] == 0 and stats[:3].sum() == faces.shape[0]
    assert direct.stats is None and int(direct.occupied) == inside.sum()


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    cases = [(vc.case("both_tiers", r), r) for r in RULES]
    tensors = [(dev(c["v"]), dev(c["f"])) for c, _ in cases]

    def run():
        out = {}
        for (c, rule), (tv, tf) in zip(cases, tensors):
            g = F.voxelize_mesh(tv, tf, c["lo"], c["step"], c["dims"], rule=rule)
            out[rule + "_bits"], out[rule + "_stats"] = g.bits, g.stats
            out[rule + "_counts"] = F.voxel_stats(g)
        return out

    first = {k: t.clone() for k, t in run().items()}          # (also loads the kernels before the capture)
    second = run()
    torch.cuda.synchronize()
    for k in first:
        assert first[k].cpu().numpy().tobytes() == second[k].cpu().numpy().tobytes(), k
    for c, rule in cases:
        assert np.array_equal(first[rule + "_bits"].cpu().numpy().view(np.uint32), c["ref"]["bits"])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = run()
    for _ in range(2):
        for t in res.values():
            t.fill_(7)                                        # every output is written by the call; the workspace carries nothing over
        g.replay()
        torch.cuda.synchronize()
        for k in first:
            assert first[k].cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("dims", [(12, 10, 9), (5, 7, 33), (3, 4, 64), (2, 3, 130)])
def test_packed_cube_operations_equal_numpy(dims):
    rng = np.random.default_rng(sum(dims))
    cube = rng.uniform(0, 0.04, dims).astype(np.float32)
    cube[0, 0, 0] = np.nan                                    # not above any iso value
    other = rng.uniform(0, 0.04, dims).astype(np.float32)
    a, b = F.voxelize_cube(dev(cube), 0.02), F.voxelize_cube(dev(other), 0.03)
    ia, ib = cube > np.float32(0.02), other > np.float32(0.03)
    assert np.array_equal(words(a), vc.pack_bits(ia)) and np.array_equal(words(b), vc.pack_bits(ib))
    dense = a.dense()
    assert dense.dtype == torch.float32 and tuple(dense.shape) == dims and np.array_equal(dense.cpu().numpy(), ia.astype(np.float32))
    assert F.voxel_stats(a, b).cpu().numpy().tolist() == vc.voxel_counts_np(ia, ib).tolist()
    assert F.voxel_stats(a).cpu().numpy().tolist() == vc.voxel_counts_np(ia).tolist()
    slot = torch.full((4,), -5, device=DEV, dtype=torch.int64)
    assert F.voxel_stats(b, a, out=slot) is slot and slot.cpu().numpy().tolist() == vc.voxel_counts_np(ib, ia).tolist()
    with pytest.raises(L.GpnerfError, match="differ"):
        F.voxel_stats(a, F.voxelize_cube(dev(np.zeros((2, 2, 2), np.float32))))


def test_contains_equals_numpy():
    c = vc.case("anisotropic", "parity")
    grid = voxelize(c, "parity")
    rng = np.random.default_rng(8)
    lo, step, dims = c["lo"], c["step"], np.array(c["dims"])
    inside_box = lo + rng.uniform(-2, dims + 1, (4000, 3)) * step
    # lattice points themselves, points half-way between two (rint: half to even), points outside, and values that are not finite
    ijk = rng.integers(0, dims, (500, 3))
    on = lo + ijk * step
    half = lo + (ijk + np.array([0.5, 0.0, 0.0])) * step
    odd = mm.f32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [-1e30, 0, 0], [0, 0, 1e38]])
    pts = mm.f32(np.concatenate([inside_box, on, half, odd]))
    got = grid.contains(dev(pts)).cpu().numpy()
    want = vc.contains_np(c["ref"]["occ"], lo, step, pts)
    print(f"contains: {int(want.sum())} of {len(pts)} inside, {int((got != want).sum())} differ")
    assert got.dtype == np.uint8 and np.array_equal(got, want) and 100 < want.sum() < len(pts) - 100
    assert not got[-len(odd):].any()
    assert grid.contains(torch.zeros((0, 3), device=DEV)).shape == (0,)
    # exact half-way points on a unit lattice: 2.5 -> 2, 3.5 -> 4
    box = voxelize(vc.case("box_nz9", "parity"), "parity")
    halves = mm.f32([[1.5, 3.0, 2.0], [2.5, 3.0, 2.0], [6.5, 3.0, 2.0], [7.5, 3.0, 2.0], [2.0, 2.5, 2.0], [2.0, 3.0, 5.5], [2.0, 3.0, 1.5]])
    assert box.contains(dev(halves)).cpu().numpy().tolist() == [1, 1, 1, 0, 0, 0, 1]


def test_a_voxelised_closed_mesh_meshes_watertight_again():
    """a scan as a cube: voxelise, unpack, marching cubes at 0.5 -> a closed, oriented surface (frame.mesh_topology); and cube_clean
    takes the same cube"""
    c = vc.case("anisotropic", "nonzero")
    grid = voxelize(c, "nonzero")
    cube = grid.dense()
    v, f = F.marching_cubes(cube, 0.5)
    topo = F.read_mesh_topology(F.mesh_topology(f, int(v.shape[0])))
    print(f"re-meshed: {v.shape[0]} vertices, {f.shape[0]} faces, {topo}")
    assert f.shape[0] > 1000 and topo["watertight"] and topo["euler"] == 2
    again = F.voxelize_mesh(v, f, (0, 0, 0), (1, 1, 1), c["dims"], rule="nonzero")
    assert np.array_equal(words(again), c["ref"]["bits"]), "and its voxelisation is the grid it came from"
    cleaned, stats, _ = F.cube_clean(cube, iso=0.5, keep="largest")
    assert stats.cpu().numpy()[0] == 1 and np.array_equal(cleaned.cpu().numpy(), cube.cpu().numpy())


def test_a_mesh_handed_over_whole_and_the_refusals():
    c = vc.case("box_nz9", "parity")
    whole = F.voxelize_mesh(M.Mesh(c["v"], c["f"]), None, c["lo"], c["step"], c["dims"])
    assert whole.bits.is_cuda and np.array_equal(words(whole), c["ref"]["bits"]) and whole.cell_volume == 1.0
    with pytest.raises(L.GpnerfError, match="dims"):
        F.voxelize_mesh(dev(c["v"]), dev(c["f"]), c["lo"], c["step"], (12, 0, 9))
    with pytest.raises(L.GpnerfError, match="step"):
        F.voxelize_mesh(dev(c["v"]), dev(c["f"]), c["lo"], (1, -1, 1), c["dims"])


# ---- MeshEvaluator(volume=True)

PAD = ev.MeshEvaluator.PAD
AXES = [np.linspace(-0.6, 0.6, 13).astype(np.float32), np.linspace(-0.5, 0.7, 13).astype(np.float32), np.linspace(-0.6, 0.6, 13).astype(np.float32)]
DIMS = (13 + 2 * PAD,) * 3


def _lattice():
    ax = [a.astype(np.float64) for a in AXES]
    step = np.array([(a[-1] - a[0]) / (len(a) - 1) for a in ax])
    return np.array([a[0] for a in ax]) - PAD * step, step


def _box_frames(shift=(0.0, 0.0, 0.0)):
    """per frame: a geometry-mode output whose mesh is a box in index units of the padded 33^3 cube, and a batch whose gt_mesh is the
    same box (moved by `shift` index units) in the axes' frame"""
    out = []
    for i in range(2):
        lo, hi = (PAD + 2.25, PAD + 3.25, PAD + 1.5 + i), (PAD + 9.25, PAD + 8.25, PAD + 10.5)
        pred = M.Mesh(*vc.box_mesh(lo, hi))
        moved = M.Mesh(*vc.box_mesh(tuple(np.add(lo, shift)), tuple(np.add(hi, shift))))
        output = {"cube": np.pad(np.zeros((13, 13, 13), np.float32), PAD), "mesh": pred, "axes": AXES}
        out.append((output, {"frame_index": torch.tensor([i]), "gt_mesh": moved.to_lattice_frame(AXES, PAD)}, pred, moved))
    return out


def test_mesh_evaluator_volume_end_to_end(tmp_path):
    # the frame's own mesh as the scan: the same solid, whatever the frame conversion rounds (no crossing is near a lattice index)
    e = ev.MeshEvaluator(str(tmp_path / "a"), 0.02, metric_samples=2000, volume=True)
    assert e.volume_rule == "nonzero" and not e.has_mesh_metrics
    for output, batch, _, _ in _box_frames():
        e.evaluate(output, batch)
    assert e.has_mesh_metrics
    s = e.summarize()
    assert s["volume_iou"] == 1.0 and s["per_frame"]["volume_iou"] == [1.0, 1.0] and s["per_frame"]["volume_frame_index"] == [0, 1]
    assert s["volume_open_columns_pred"] == 0 and s["volume_open_columns_gt"] == 0 and s["volume_pred"] == s["volume_gt"] > 0
    assert "chamfer" in s, "beside the surface metrics of the same frames"
    table = np.load(tmp_path / "a" / "volume_metrics.npy")
    assert len(table) == 2 and table["iou"].tolist() == [1.0, 1.0] and (table["points_pred"] == table["points_both"]).all()
    assert sorted(os.listdir(tmp_path / "a")) == ["mesh_metrics.npy", "pts", "volume_metrics.npy"]
    assert e.summarize() == {} and not e.has_mesh_metrics     # reset

    # a scan moved by (2, 1, 0) lattice steps: the restatement's counts, on the lattices the evaluator is documented to use
    lo, step = _lattice()
    for rule in RULES:
        b = ev.MeshEvaluator(str(tmp_path / rule), 0.02, metric_samples=2000, volume=True, volume_rule=rule)
        expect = []
        for output, batch, pred, moved in _box_frames(shift=(2.0, 1.0, 0.0)):
            b.evaluate(output, batch)
            p = vc.voxelize_np(pred.vertices, pred.faces, (0, 0, 0), (1, 1, 1), DIMS, rule)
            g = vc.voxelize_np(mm.f32(batch["gt_mesh"].vertices), batch["gt_mesh"].faces, lo, step, DIMS, rule)
            assert p["margin"] > 1e-3 and g["margin"] > 1e-3
            expect.append(F.read_volume_metrics(vc.voxel_counts_np(p["occ"], g["occ"]), step))
        got = b.summarize()
        assert got["per_frame"]["volume_iou"] == [r["iou"] for r in expect] and got["volume_iou"] == float(np.mean([r["iou"] for r in expect]))
        assert got["per_frame"]["volume_pred"] == [r["volume_a"] for r in expect] and got["per_frame"]["volume_gt"] == [r["volume_b"] for r in expect]
        assert 0.3 < got["volume_iou"] < 0.7
        table = np.load(tmp_path / rule / "volume_metrics.npy")
        assert table["points_pred"].tolist() == [7 * 5 * (9 - i) for i in range(2)]


def test_volume_off_changes_nothing_and_on_without_axes_raises(tmp_path):
    output, batch, _, _ = _box_frames()[0]
    both = [ev.MeshEvaluator(str(tmp_path / name), 0.02, metric_samples=2000, volume=flag) for name, flag in (("plain", False), ("vol", True))]
    for m in both:
        m.evaluate(output, batch)
    plain, vol = (m.summarize() for m in both)
    assert not any("volume" in k for k in plain) and not any("volume" in k for k in plain["per_frame"])
    assert sorted(os.listdir(tmp_path / "plain")) == ["mesh_metrics.npy", "pts"]
    assert {k: v for k, v in vol.items() if "volume" not in k and k != "per_frame"} == {k: v for k, v in plain.items() if k != "per_frame"}
    assert {k: v for k, v in vol["per_frame"].items() if "volume" not in k} == plain["per_frame"]
    assert np.load(tmp_path / "plain" / "mesh_metrics.npy").tobytes() == np.load(tmp_path / "vol" / "mesh_metrics.npy").tobytes()
    on = ev.MeshEvaluator(str(tmp_path / "on"), 0.02, metric_samples=2000, volume=True)
    pts = torch.from_numpy(np.stack(np.meshgrid(*AXES, indexing="ij"), axis=-1))[None]
    with pytest.raises(L.GpnerfError, match="axes"):
        on.evaluate({"cube": output["cube"], "mesh": output["mesh"]}, dict(batch, pts=pts))
    off = ev.MeshEvaluator(str(tmp_path / "none"), 0.02, volume=True)
    off.evaluate(output, {"frame_index": batch["frame_index"]})     # no gt_mesh: nothing is enqueued
    assert not off.has_mesh_metrics and off.summarize() == {}
