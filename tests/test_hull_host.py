"""Host: the dense renderer's geometry mode without a GPU -- the visual hull's numpy restatement (tests/hull_cases.py, the
specification of gpnerf_visual_hull) against the reference's own prepare_inside_pts runs (tests/golden/hull/*.npz), the dataset's
lattice axes, the mesh evaluator, and the evaluation loop's `evaluator` argument."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import hull_cases as hc

F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
ev = importlib.import_module("gp-nerf_amd.evaluator")


def test_the_four_hull_fixtures_are_there():
    assert hc.hull_case_names() == ["hull_body", "hull_close", "hull_eight", "hull_one"]


@pytest.mark.parametrize("name", hc.hull_case_names())
def test_restatement_is_the_reference_hull(name):
    """prepare_inside_pts as the reference ran it == the plain-order float64 restatement, outside the near-tie points (<= 1e-4)"""
    z, meta, axes = hc.load_hull(name)
    got, tie, converted = hc.hull_np(axes, z["masks"], z["cams"])
    left_out = hc.compare_outside_ties(got, z["inside"], tie)
    assert left_out == meta["near_ties"] and converted == meta["converted"]
    assert tuple(got.shape) == tuple(meta["dims"]) and z["masks"].shape[0] == meta["n_views"]
    print(f"{name}: {got.size} points, {left_out} left out, {converted} out-of-range conversions, values {meta['counts']}")


def test_hull_fixtures_show_what_they_are_for():
    z, meta, _ = hc.load_hull("hull_body")
    assert set(np.unique(z["inside"])) == {0, 1, 100} and meta["n_views"] == 4          # the sticky border value is an output value
    assert hc.load_hull("hull_one")[1]["n_views"] == 1
    assert hc.load_hull("hull_close")[1]["converted"] > 0                             # INT32_MIN conversions happen
    z, meta, _ = hc.load_hull("hull_eight")
    assert meta["n_views"] == 8 and meta["dims"] == [3, 5, 130]


def test_pixel_conversion_quirk():
    """what does not fit int32 after rounding, and what is not finite, becomes INT32_MIN and clips to 0 -- not to the far edge"""
    v = np.array([0.5, 1.5, 2.5, -0.5, -3.0, 7.49, 1e6, 2147483647.4, 2147483647.5, 2.0 ** 31, -2.0 ** 31, -2.0 ** 31 - 1, 1e300, np.inf, -np.inf, np.nan])
    q, bad = hc.pixel_of(v, 9)
    assert q.tolist() == [0, 2, 2, 0, 0, 7, 9, 9, 0, 0, 0, 0, 0, 0, 0, 0]
    assert bad.tolist() == [False] * 8 + [True] * 8


@pytest.mark.parametrize("lo, hi, step", [(-0.3, 0.3, 0.005), (-0.3, 0.3024, 0.005), (0.0137, 0.2911, 0.005), (-1.0, 1.0, 0.25),
                                          (0.1, 0.1, 0.005), (-0.123, 0.377, 0.0075)])
def test_dataset_lattice_axis(lo, hi, step):
    """ZjumocapDataset.py:397-402 with the reference era's promotion: the stop is float64(hi) + step, not rounded to float32"""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    a = F.dataset_lattice_axis(lo32, hi32, step)
    l64, stop = np.float64(lo32), np.float64(hi32) + np.float64(step)
    n = int(np.ceil((stop - l64) / np.float64(step)))
    assert a.dtype == np.float32 and len(a) == n
    assert a[0] == lo32 and a[-1] == np.float32(l64 + (n - 1) * np.float64(step))
    assert np.float64(a[-1]) < stop + 1e-6 and l64 + n * np.float64(step) >= stop          # the last value before the stop
    for i in (0, 1, n // 2, n - 1):
        assert a[i] == np.float32(l64 + i * np.float64(step))
    assert np.array_equal(a, (l64 + np.arange(n, dtype=np.float64) * np.float64(step)).astype(np.float32))


def test_dataset_lattice_axis_lengths_on_and_off_the_step():
    # a bound on a multiple of the step (exactly representable): arange's half-open stop hi + step keeps hi itself
    a = F.dataset_lattice_axis(np.float32(-1.0), np.float32(1.0), 0.25)
    assert len(a) == 9 and a[0] == -1.0 and a[-1] == 1.0
    # off a multiple: the last value is the last one below hi + step, past hi
    b = F.dataset_lattice_axis(np.float32(0.0), np.float32(0.9), 0.25)
    assert len(b) == 5 and b[-1] == 1.0
    # a degenerate box still has its one point
    c = F.dataset_lattice_axis(np.float32(0.5), np.float32(0.5), 0.25)
    assert len(c) == 1 and c[0] == 0.5
    axes = F.dataset_lattice_axes(np.array([[-1.0, 0.0, 0.5], [1.0, 0.9, 0.5]], np.float32), (0.25, 0.25, 0.25))
    assert [len(x) for x in axes] == [9, 5, 1] and all(x.dtype == np.float32 for x in axes)


def _hand_made():
    rng = np.random.default_rng(4)
    axes = [np.linspace(-0.1, 0.1, 5).astype(np.float32), np.linspace(0.2, 0.5, 7).astype(np.float32), np.linspace(1.0, 1.3, 4).astype(np.float32)]
    inner = rng.uniform(0, 0.04, (5, 7, 4)).astype(np.float32)
    cube = np.pad(inner, 10, constant_values=1.0)           # padding above the threshold: the crop must take it away
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).astype(np.float32)
    mesh = M.Mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64), np.array([[0, 1, 2]]))
    return axes, inner, cube, pts, mesh


def test_mesh_evaluator_saves_the_cropped_points_above_the_threshold(tmp_path):
    axes, inner, cube, pts, mesh = _hand_made()
    th = 0.02
    want = pts[inner > th]
    assert 0 < len(want) < inner.size
    out = {"cube": cube, "mesh": mesh, "axes": axes}
    a = ev.MeshEvaluator(str(tmp_path / "a"), th)
    a.evaluate(out, {"pts": torch.from_numpy(pts)[None], "frame_index": torch.tensor([7])})
    b = ev.MeshEvaluator(str(tmp_path / "b"), th)
    b.evaluate(out, {"frame_index": torch.tensor([7])})
    got_a, got_b = np.load(tmp_path / "a" / "pts" / "7.npy"), np.load(tmp_path / "b" / "pts" / "7.npy")
    assert got_a.dtype == np.float32 and np.array_equal(got_a, want)
    assert got_b.dtype == np.float32 and np.array_equal(got_b, want)
    assert not os.path.exists(tmp_path / "a" / "mesh")                                 # evaluate alone exports nothing
    assert a.summarize() == {} and b.summarize() == {}


def test_mesh_evaluator_ply_names(tmp_path):
    axes, inner, cube, pts, mesh = _hand_made()
    out = {"cube": cube, "mesh": mesh, "axes": axes}
    e = ev.MeshEvaluator(str(tmp_path), 0.02)
    e.visualize(out, {"frame_index": torch.tensor([3])})
    e.visualize(out, {"frame_index": torch.tensor([3]), "cam_ind": torch.tensor([5])})
    assert sorted(os.listdir(tmp_path / "mesh")) == ["3.ply", "3_cam5.ply"]
    assert open(tmp_path / "mesh" / "3.ply", "rb").read(3) == b"ply"
    e2 = ev.MeshEvaluator(str(tmp_path / "x"), 0.02, export_mesh=True)
    e2.evaluate(out, {"frame_index": torch.tensor([4])})
    assert os.listdir(tmp_path / "x" / "mesh") == ["4.ply"] and os.listdir(tmp_path / "x" / "pts") == ["4.npy"]


class _FakeGeometryRender(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out, self.nerfhead = out, types.SimpleNamespace(use_rgbhead=False)
        self.prefetched = 0

    def prefetch(self, batch):                      # (its presence alone used to turn the pipeline on)
        self.prefetched += 1
        raise AssertionError("a geometry-mode renderer is not pipelined by default")

    def render(self, batch):
        return dict(self.out, rtime=0.5)


def test_evaluate_loop_uses_the_evaluator_it_is_given(tmp_path, monkeypatch):
    axes, inner, cube, pts, mesh = _hand_made()
    cfg = types.SimpleNamespace(test=types.SimpleNamespace(test_seq="s"), head=types.SimpleNamespace(rgb=types.SimpleNamespace(use_rgbhead=False)))
    made = []

    class Spy(ev.Evaluator):
        def __init__(self, *a):
            made.append(type(self).__name__)
            super().__init__(*a)

    monkeypatch.setattr(ev, "Evaluator", Spy)
    monkeypatch.delenv("GPNERF_DEVICE_METRICS", raising=False)
    model = _FakeGeometryRender({"cube": cube, "mesh": mesh, "axes": axes})
    e = ev.MeshEvaluator(str(tmp_path), 0.02, export_mesh=True)
    loader = [{"frame_index": torch.tensor([i])} for i in (0, 1)]
    res = ev.evaluate_loop(model, loader, cfg, quiet=True, evaluator=e)
    assert made == [] and res["count"] == 2 and res["total_time"] == 1.0 and res["metrics"] is None
    assert res["mse"] == [] and res["psnr"] == [] and res["ssim"] == []
    assert sorted(os.listdir(tmp_path / "pts")) == ["0.npy", "1.npy"] and sorted(os.listdir(tmp_path / "mesh")) == ["0.ply", "1.ply"]
    # without the argument the loop builds what it built before, whatever use_rgbhead says
    out = ev.evaluate_loop(torch.nn.Identity(), [], cfg, quiet=True, pipeline=False)
    assert made == ["Spy"] and out["count"] == 0 and out["mse"] == []
