"""GPU: the mesh rasteriser (gpnerf_raster.hip) against the numpy restatement of include/gpnerf_hip.h (tests/raster_cases.py): depth
bits, face ids, statistics and silhouette counts EQUAL -- both sides evaluate the same unfused float64 expressions and exact int64
edge functions, and the cases hold no near-tie snap --, attribute images bit-equal, two runs and a graph replay identical, and
MeshEvaluator(silhouette=True) end to end.  Images of 40 x 24 and 130 x 70, one and three views."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import mesh_metric_cases as mm
import raster_cases as rc

pytestmark = pytest.mark.gpu
F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
L = importlib.import_module("gp-nerf_amd._lib")
ev = importlib.import_module("gp-nerf_amd.evaluator")
DEV = "cuda:0"
SHAPES = [("small", 1), ("large", 3)]
# every case at both image sizes and both view counts; the 5 120-face sphere crosses them the other way round, which keeps the
# restatement's brute force (faces x pixels x views) at a second or so
RUNS = [(n, s, v) for n in rc.NAMES for s, v in ([("small", 3), ("large", 1)] if n == "icosphere4" else SHAPES)]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the cases' arrays are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def draw(c, **kw):
    res = F.rasterize_mesh(dev(c["v"]), dev(c["f"]), c["Ks"], c["RTs"], c["H"], c["W"], z_near=rc.Z_NEAR, **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in res.items()}


def assert_equal_to_restatement(what, got, ref):
    diff = bits(got["depth"]) != bits(ref["depth"])
    wrong_id = got["face_id"] != ref["face_id"]
    print(f"{what}: stats {got['stats'].tolist()} (restatement {ref['stats'].tolist()}), depth words that differ {int(diff.sum())}, "
          f"face ids that differ {int(wrong_id.sum())} of {diff.size}")
    assert got["stats"].dtype == np.int64 and np.array_equal(got["stats"], ref["stats"]), what
    assert not wrong_id.any(), (what, np.argwhere(wrong_id)[:5].tolist())
    assert not diff.any(), (what, np.argwhere(diff)[:5].tolist())


@pytest.mark.parametrize("name,size,n_views", RUNS)
def test_depth_face_id_and_stats_equal_the_restatement(name, size, n_views):
    c = rc.case(name, size, n_views)
    got = draw(c)
    assert_equal_to_restatement(f"{name} {size} x{n_views}", got, c["ref"])
    ref = c["ref"]
    if name == "zero_faces":
        assert not got["stats"].any() and (got["face_id"] == -1).all() and np.isposinf(got["depth"]).all()
    if name in ("large_faces", "both_tiers"):               # (the case is what it says: a face beyond the small tier's box, drawn)
        assert (ref["face_id"][0] == (0 if name == "large_faces" else len(c["f"]) - 2)).sum() > 256
    if name == "icosphere4":
        # (every face is usable; at 40 x 24 a face is a fraction of a pixel and a few snap to zero area)
        assert len(c["f"]) == 5120 and (ref["stats"][:, :3].sum(axis=1) == 5120).all() and not ref["stats"][:, 1].any()
        assert (ref["stats"][:, 0] > 5000).all()
    if name == "tie_cube":
        assert (got["face_id"] < 12).all() and (got["face_id"] >= 0).any()
    if name == "degenerate_mix":
        assert (ref["stats"][:, 1] == 4).all() and (ref["stats"][:, 2] >= 1).all()
    if name == "near_and_guard":
        assert ref["stats"][0].tolist()[:3] == [2, 3, 0]


@pytest.mark.parametrize("size,n_views", SHAPES)
def test_optional_outputs_and_a_mesh_handed_over_whole(size, n_views):
    c = rc.case("both_tiers", size, n_views)
    only_depth = draw(c, want=("depth",))
    assert set(only_depth) == {"depth", "stats"} and np.array_equal(bits(only_depth["depth"]), bits(c["ref"]["depth"]))
    only_id = draw(c, want=("face_id",))
    assert set(only_id) == {"face_id", "stats"} and np.array_equal(only_id["face_id"], c["ref"]["face_id"])
    assert np.array_equal(only_id["stats"], c["ref"]["stats"])
    whole = F.rasterize_mesh(M.Mesh(c["v"], c["f"]), None, c["Ks"], c["RTs"], c["H"], c["W"], z_near=rc.Z_NEAR)
    assert whole["face_id"].is_cuda and np.array_equal(whole["face_id"].cpu().numpy(), c["ref"]["face_id"])


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("name,size,n_views", [("icosphere2", "small", 1), ("both_tiers", "large", 3), ("pixel_centres", "small", 1),
                                               ("near_and_guard", "large", 3)])
def test_attribute_images_equal_the_restatement(name, size, n_views, channels):
    c = rc.case(name, size, n_views)
    attrs = rc.colours_of(c["v"], channels)
    bg = [0.25, 0.5, 0.75][:channels] if channels > 1 else -1.0
    got = draw(c, attributes=dev(attrs if channels > 1 else attrs.reshape(-1)), background=bg)
    ref = rc.interpolate_np(c["ref"]["face_id"], c["v"], c["f"], c["cams"], c["H"], c["W"], attrs, bg)
    assert got["image"].shape == (n_views, c["H"], c["W"], channels) and got["image"].dtype == np.float32
    diff = bits(got["image"]) != bits(ref)
    print(f"{name} C={channels}: image words that differ {int(diff.sum())} of {diff.size}")
    assert not diff.any()
    empty = c["ref"]["face_id"] < 0
    assert empty.any() or name == "both_tiers"               # (whose background face spans the image)
    assert (got["image"][empty] == np.broadcast_to(np.asarray(bg, np.float32), (channels,))).all()
    covered = ~empty
    assert (got["image"][covered] >= 0).all() and (got["image"][covered] <= 1).all(), "a convex combination of attributes in [0, 1]"


def test_silhouette_counts_equal_the_restatement():
    c = rc.case("icosphere2", "large", 3)
    fid = c["ref"]["face_id"]
    masks = np.zeros(fid.shape, np.uint8)
    masks[:, :, 3:] = fid[:, :, :-3] >= 0                     # the silhouette itself, 3 columns to the right
    masks[2] = 0                                              # a view with nothing to draw
    masks[:, 30:34] = 100                                     # a band of border values
    got = F.silhouette_stats(dev(fid), dev(masks)).cpu().numpy()
    ref = rc.silhouette_np(fid, masks)
    print("silhouette counts", got.tolist())
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert (ref[:, 4] == 4 * c["W"]).all() and ref[2, 1] == 0 and 0 < ref[0, 2] < ref[0, 0]


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    c = rc.case("both_tiers", "large", 3)
    tv, tf, attrs = dev(c["v"]), dev(c["f"]), dev(rc.colours_of(c["v"], 3))
    masks = dev((c["ref"]["face_id"] >= 0).astype(np.uint8))

    def run():
        res = F.rasterize_mesh(tv, tf, c["Ks"], c["RTs"], c["H"], c["W"], z_near=rc.Z_NEAR, attributes=attrs, background=0.5)
        res["counts"] = F.silhouette_stats(res["face_id"], masks)
        return res

    first = {k: t.clone() for k, t in run().items()}          # (also loads the kernels before the capture)
    second = run()
    torch.cuda.synchronize()
    for k in first:
        assert first[k].cpu().numpy().tobytes() == second[k].cpu().numpy().tobytes(), k
    assert np.array_equal(first["face_id"].cpu().numpy(), c["ref"]["face_id"])
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


# ---- MeshEvaluator(silhouette=True)

PAD = ev.MeshEvaluator.PAD
AXES = [np.linspace(-0.6, 0.6, 13).astype(np.float32), np.linspace(-0.5, 0.7, 13).astype(np.float32), np.linspace(-0.6, 0.6, 13).astype(np.float32)]


def _sphere_frames(n_frames=2, n_views=3, size="large"):
    """per frame: the output of a geometry-mode render -- an icosphere in index units of the padded cube, the axes -- and a batch with
    cameras and the masks the RESTATEMENT draws from the same sphere in the axes' frame"""
    H, W = rc.SIZES[size]
    Ks, RTs = rc.orbit_cameras(H, W, n_views, radius=0.6, distance=3.0, seed=5)
    out = []
    for i in range(n_frames):
        sv, sf = mm.icosphere(2)
        pred = M.Mesh(mm.f32((4.0 + 0.5 * i) * sv.astype(np.float64) + (PAD + 6.0)), sf)      # index units: centre of the 13^3 lattice
        placed = pred.to_lattice_frame(AXES, PAD)
        cams = rc.hull_cases.cams_of(Ks, RTs)
        rc.assert_no_near_ties(mm.f32(placed.vertices), placed.faces, cams)
        ref = rc.rasterize_np(mm.f32(placed.vertices), placed.faces, cams, H, W)
        masks = (ref["face_id"] >= 0).astype(np.uint8)
        cube = np.pad(np.zeros((13, 13, 13), np.float32), PAD)
        output = {"cube": cube, "mesh": pred, "axes": AXES}
        batch = {"frame_index": torch.tensor([i]), "hull_masks": dev(masks)[None], "hull_Ks": torch.from_numpy(Ks)[None].to(DEV),
                 "hull_RTs": torch.from_numpy(RTs)[None].to(DEV)}
        out.append((output, batch, ref))
    return out


def test_mesh_evaluator_silhouette_end_to_end(tmp_path):
    frames = _sphere_frames()
    e = ev.MeshEvaluator(str(tmp_path / "a"), 0.02, silhouette=True)
    assert not e.has_mesh_metrics
    for output, batch, _ in frames:
        e.evaluate(output, batch)
    assert e.has_mesh_metrics
    s = e.summarize()
    assert s["silhouette_iou"] == 1.0 and s["silhouette_precision"] == 1.0 and s["silhouette_recall"] == 1.0
    assert s["per_frame"]["silhouette_iou"] == [1.0, 1.0] and s["per_frame"]["silhouette_frame_index"] == [0, 1]
    table = np.load(tmp_path / "a" / "silhouette_metrics.npy")
    assert len(table) == 2 and table["frame_index"].tolist() == [0, 1] and table["iou"].tolist() == [1.0, 1.0]
    assert table["iou_per_view"].shape == (2, 3) and (table["views"] == 3).all()
    assert sorted(os.listdir(tmp_path / "a")) == ["pts", "silhouette_metrics.npy"]
    assert e.summarize() == {} and not e.has_mesh_metrics     # reset

    # the masks shifted by 3 columns, with a band of border values: the restatement's counts
    b = ev.MeshEvaluator(str(tmp_path / "b"), 0.02, silhouette=True)
    expect = []
    for output, batch, ref in frames:
        covered = ref["face_id"] >= 0
        masks = np.zeros(covered.shape, np.uint8)
        masks[:, :, 3:] = covered[:, :, :-3]
        masks[:, 33:37] = 100
        b.evaluate(output, dict(batch, hull_masks=dev(masks)[None]))
        expect.append(F.read_silhouette_metrics(rc.silhouette_np(ref["face_id"], masks)))
    got = b.summarize()
    for k in ("iou", "precision", "recall"):
        assert got["per_frame"][f"silhouette_{k}"] == [r[k] for r in expect], k
        assert got[f"silhouette_{k}"] == float(np.mean([r[k] for r in expect]))
    assert 0.5 < got["silhouette_iou"] < 1.0
    table = np.load(tmp_path / "b" / "silhouette_metrics.npy")
    assert table["iou_per_view"].tolist() == [r["per_view"]["iou"] for r in expect]
    assert (table["ignored_per_view"] == 4 * rc.SIZES["large"][1]).all()


def test_the_loop_passes_a_silhouette_evaluator_through(tmp_path):
    frames = _sphere_frames()

    class Render(torch.nn.Module):
        nerfhead = types.SimpleNamespace(use_rgbhead=False)
        at = 0

        def render(self, batch):
            self.at += 1
            return dict(frames[self.at - 1][0], rtime=0.25)

    cfg = types.SimpleNamespace(test=types.SimpleNamespace(test_seq="s"), head=types.SimpleNamespace(rgb=types.SimpleNamespace(use_rgbhead=False)))
    e = ev.MeshEvaluator(str(tmp_path), 0.02, silhouette=True)
    res = ev.evaluate_loop(Render(), [b for _, b, _ in frames], cfg, device=DEV, quiet=True, evaluator=e)
    assert res["count"] == 2 and res["metrics"]["silhouette_iou"] == 1.0 and os.path.exists(tmp_path / "silhouette_metrics.npy")


def test_silhouette_off_changes_nothing_and_on_without_axes_raises(tmp_path):
    frames = _sphere_frames(n_frames=1)
    output, batch, _ = frames[0]
    off = ev.MeshEvaluator(str(tmp_path / "off"), 0.02)
    off.evaluate(output, batch)                               # masks and cameras in the batch, the option off
    assert not off.has_mesh_metrics and off.summarize() == {} and os.listdir(tmp_path / "off") == ["pts"]
    # with a gt_mesh: the geometry metrics' keys and file, nothing of the silhouette
    gt = output["mesh"].to_lattice_frame(AXES, PAD)
    both = [ev.MeshEvaluator(str(tmp_path / name), 0.02, metric_samples=2000, silhouette=flag) for name, flag in (("plain", False), ("sil", True))]
    for m in both:
        m.evaluate(output, dict(batch, gt_mesh=gt))
    plain, sil = (m.summarize() for m in both)
    assert not any("silhouette" in k for k in plain) and not any("silhouette" in k for k in plain["per_frame"])
    assert sorted(os.listdir(tmp_path / "plain")) == ["mesh_metrics.npy", "pts"]
    assert sorted(os.listdir(tmp_path / "sil")) == ["mesh_metrics.npy", "pts", "silhouette_metrics.npy"]
    assert {k: v for k, v in sil.items() if "silhouette" not in k and k != "per_frame"} == {k: v for k, v in plain.items() if k != "per_frame"}
    assert {k: v for k, v in sil["per_frame"].items() if "silhouette" not in k} == plain["per_frame"] and sil["silhouette_iou"] == 1.0
    assert np.load(tmp_path / "plain" / "mesh_metrics.npy").tobytes() == np.load(tmp_path / "sil" / "mesh_metrics.npy").tobytes()
    # on, but the output has no axes (the inference renderer's render_mesh): the error names the key
    on = ev.MeshEvaluator(str(tmp_path / "on"), 0.02, silhouette=True)
    pts = torch.from_numpy(np.stack(np.meshgrid(*AXES, indexing="ij"), axis=-1))[None]
    with pytest.raises(L.GpnerfError, match="axes"):
        on.evaluate({"cube": output["cube"], "mesh": output["mesh"]}, dict(batch, pts=pts))
    # on, and a batch without masks: nothing is enqueued
    on.evaluate(output, {"frame_index": batch["frame_index"]})
    assert not on.has_mesh_metrics and on.summarize() == {}
