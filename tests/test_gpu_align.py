"""GPU: registering a mesh onto a scan on the device (csrc/gpnerf_align.hip) against the numpy restatement of include/gpnerf_hip.h
(tests/align_cases.py): the sums bit for bit, the solved matrices within 2^-32, transform_points within a float32 ulp, the loop
(frame.align_mesh) under the host test's bound, two runs and a graph replay with the same bytes, mesh_metrics(align="rigid") and
MeshEvaluator(align="rigid") end to end.

Bounds, none taken from what the kernels give: the sums are exact conversions, products and additions in one stated association, so
they compare as bits; the solves differ from the restatement at most by a one-ulp sqrt or division in fewer than 10^3 operations on
systems of cond <= 10^3 (asserted in tests/test_align_host.py): under 10^6 2^-53 < 2^-32; the loop's bound is 2^-18 max |coordinate|."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import align_cases as ac
import mesh_metric_cases as mm

pytestmark = pytest.mark.gpu
F = importlib.import_module("gp-nerf_amd.frame")
M = importlib.import_module("gp-nerf_amd.mesh")
L = importlib.import_module("gp-nerf_amd._lib")
ev = importlib.import_module("gp-nerf_amd.evaluator")
DEV = "cuda:0"
INF = float("inf")
TOL = 2.0 ** -32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


def differing(a, b):
    a, b = np.ascontiguousarray(a, np.float64).reshape(-1), np.ascontiguousarray(b, np.float64).reshape(-1)
    return int((a.view(np.int64) != b.view(np.int64)).sum())


def ws_doubles(ws):
    return ws.cpu().numpy().view(np.float64)


def ws_part(ws, name, count):
    at = L.ALIGN_WS[name]
    return ws_doubles(ws)[at:at + count]


def slot_of(t):
    s = t.cpu().numpy()
    return {"M": s[L.XFORM_M:L.XFORM_M + 12].reshape(3, 4), "scale": s[L.XFORM_SCALE], "status": int(s[L.XFORM_STATUS]), "used": int(s[L.XFORM_USED]),
            "skipped": int(s[L.XFORM_SKIPPED]), "trimmed": int(s[L.XFORM_TRIMMED]), "wsum": s[L.XFORM_WSUM], "rms": s[L.XFORM_RMS],
            "pivot": s[L.XFORM_PIVOT:L.XFORM_PIVOT + 3]}


# ---------------------------------------------------------------- rigid_fit

SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 40000)


@pytest.mark.parametrize("n", SIZES)
def test_rigid_fit_matches_the_restatement(n):
    """the wavefront, block and grid-stride edges; with and without weights and scale; NaN and inf coordinates, zero, negative and NaN
    weights among the pairs"""
    src, dst, w = ac.pair_set(n, seed=100 + n, dirty=True, scale=1.3)
    tsrc, tdst, tw = dev(src), dev(dst), dev(w)
    diff_total = 0
    for weights in (False, True):
        for scale in (False, True):
            ref = ac.rigid_fit(src, dst, w if weights else None, scale)
            ws = F.align_workspace(DEV)
            ws.fill_(0xAB)
            slot = F.rigid_fit(tsrc, tdst, tw if weights else None, scale=scale, workspace=ws)
            torch.cuda.synchronize()
            got = slot_of(slot)
            what = f"n {n} weights {weights} scale {scale}"
            assert (got["used"], got["skipped"], got["status"], got["trimmed"]) == (ref["used"], ref["skipped"], ref["status"], 0), what
            assert same_bits(ws_part(ws, "sums1", 7), ref["sums1"]), what
            assert same_bits(ws_part(ws, "centroids", 6), ref["centroids"]), what
            assert same_bits(ws_part(ws, "sums2", 11), ref["sums2"]), what          # S, sum w |a|^2, and RMS^2 W
            assert same_bits(got["wsum"], ref["wsum"]) and same_bits(got["pivot"], ref["pivot"]), what
            assert np.isfinite(got["M"]).all() and np.isfinite(got["scale"]), what
            assert np.abs(got["M"] - ref["M"]).max() <= TOL and abs(got["scale"] - ref["scale"]) <= TOL, what
            if ref["used"]:
                assert abs(got["rms"] - ref["rms"]) <= TOL * max(1.0, ref["rms"]), what
            else:
                assert np.isnan(got["rms"]), what
            if ref["status"] != ac.OK:
                assert np.array_equal(got["M"], ac.IDENTITY) and got["scale"] == 1.0, what
            if not scale:
                assert got["scale"] == 1.0
            diff_total += differing(got["M"], ref["M"]) + differing(got["scale"], ref["scale"])
    print(f"rigid_fit n {n}: {diff_total} of {4 * 13} entries of M and SCALE differ from the restatement in their bits")


def test_rigid_fit_degenerate_sets_and_the_slot_argument():
    same = dev(np.tile(np.float32([[1, 2, 3]]), (50, 1)))
    other = dev(ac.pair_set(50, 2)[0])
    slot = torch.full((L.XFORM_DOUBLES,), float("nan"), device=DEV, dtype=torch.float64)
    assert F.rigid_fit(same, other, out=slot) is slot
    got = slot_of(slot)
    assert got["status"] == ac.SINGULAR and np.array_equal(got["M"], ac.IDENTITY) and not np.isnan(slot.cpu().numpy()).any()
    assert slot_of(F.rigid_fit(other, same))["status"] == ac.SINGULAR
    # coplanar pairs are well defined
    rng = np.random.default_rng(5)
    src = mm.f32(np.concatenate([rng.normal(size=(300, 2)), np.zeros((300, 1))], axis=1))
    dst = mm.f32(src.astype(np.float64) @ ac.rotation((1, 2, 3), 40.0).T + [0.3, -0.2, 0.5])
    ref, got = ac.rigid_fit(src, dst), slot_of(F.rigid_fit(dev(src), dev(dst)))
    assert got["status"] == ref["status"] == ac.OK and np.abs(got["M"] - ref["M"]).max() <= TOL
    with pytest.raises(L.GpnerfError):
        F.rigid_fit(same, other[:10])


# ---------------------------------------------------------------- transform_points

def test_transform_points_matches_the_restatement():
    rng = np.random.default_rng(8)
    pts = mm.f32(rng.normal(size=(1000, 3)) * [10, 3, 1])
    pts[5, 0], pts[77, 2], pts[300, 1] = np.nan, np.inf, -np.inf
    Mx = np.hstack([1.7 * ac.rotation((1, -2, 0.5), 33.0), [[10.0], [-5.0], [3.0]]])
    slot = F.align_init(dev(pts), init=Mx)
    got_slot = slot_of(slot)
    assert same_bits(got_slot["M"], Mx) and abs(got_slot["scale"] - 1.7) < 1e-14 and got_slot["status"] == ac.OK
    assert got_slot["used"] == 997 and got_slot["skipped"] == 3 and same_bits(got_slot["pivot"], ac.pivot_of(pts))
    tp = dev(pts)
    for vectors in (False, True):
        ref = ac.transform_points(pts, Mx, got_slot["scale"], vectors)
        got = F.transform_points(tp, slot, vectors=vectors).cpu().numpy()
        bad = ~np.isfinite(pts).all(axis=1)
        assert np.isnan(got[bad]).all() and np.isnan(ref[bad]).all() and np.isfinite(got[~bad]).all()
        ulp = np.spacing(np.abs(ref[~bad]))
        print(f"transform_points vectors {vectors}: {int((got[~bad] != ref[~bad]).sum())} of {ref[~bad].size} coordinates differ in their bits")
        assert (np.abs(got[~bad].astype(np.float64) - ref[~bad]) <= ulp).all()
        if vectors:                                          # R alone: lengths are kept, nothing is translated
            assert np.allclose(np.linalg.norm(got[~bad], axis=1), np.linalg.norm(pts[~bad], axis=1), rtol=1e-6)
    first = F.transform_points(tp, slot)
    assert F.transform_points(tp, slot, out=tp) is tp and tp.cpu().numpy().tobytes() == first.cpu().numpy().tobytes()      # in place
    empty = F.transform_points(torch.empty((0, 3), device=DEV), slot)
    assert empty.shape == (0, 3)
    # the identity by default, and an empty list has the origin for a pivot
    s0 = slot_of(F.align_init(torch.empty((0, 3), device=DEV)))
    assert np.array_equal(s0["M"], ac.IDENTITY) and s0["scale"] == 1.0 and s0["used"] == 0 and np.array_equal(s0["pivot"], np.zeros(3))


# ---------------------------------------------------------------- align_step on given arrays

@functools.lru_cache(maxsize=None)
def step_case():
    """the 15-degree loop case's first correspondences from the host restatement, with every way a pair can drop out written in, on
    the ellipsoid with a zero-area face and a face with an index out of range appended"""
    pts, (v, f), _ = ac.icp_case("15deg")
    closest, face, dist = ac.correspondences(pts, v, f)
    f = np.concatenate([f, [[0, 0, 1], [0, 1, len(v)]]]).astype(np.int32)
    face, dist, closest, pts = face.copy(), dist.copy(), closest.copy(), pts.copy()
    idx = np.arange(len(pts))
    face[idx % 50 == 1], dist[idx % 50 == 1], closest[idx % 50 == 1] = -1, np.inf, np.nan          # beyond a finite max_dist upstream
    face[idx % 50 == 2] = len(f) - 2                        # a zero-area nearest face
    face[idx % 50 == 3] = len(f) - 1                        # an invalid face
    face[idx % 50 == 4] = len(f)                            # no such face
    dist[idx % 50 == 5] = np.nan
    pts[idx % 50 == 6, 1] = np.nan
    closest[idx % 50 == 7, 2] = np.inf
    dist[idx % 50 == 8] = -np.inf
    return pts, closest, face, dist, v, f


@pytest.mark.parametrize("max_dist", [INF, 0.08])
def test_align_step_matches_the_restatement(max_dist):
    pts, closest, face, dist, v, f = step_case()
    M0 = np.hstack([ac.rotation((0, 0, 1), 1.0), [[0.01], [0.0], [-0.01]]])
    slot = F.align_init(dev(pts), init=M0)
    pivot = slot_of(slot)["pivot"].copy()
    assert same_bits(pivot, ac.pivot_of(pts))
    ref = ac.align_step(pts, closest, face, dist, v, f, max_dist, M0, pivot)
    if max_dist == INF:
        assert ref["trimmed"] == 0 and ref["skipped"] == 160 and ref["used"] == 840
    else:
        assert 100 < ref["trimmed"] < 800 and ref["used"] > 100 and ref["used"] + ref["trimmed"] + ref["skipped"] == 1000
    ws = F.align_workspace(DEV)
    ws.fill_(0xAB)
    hist = torch.full((4,), -1.0, device=DEV, dtype=torch.float64)
    near = {"closest": dev(closest), "face": dev(face), "dist": dev(dist)}
    assert F.align_step(dev(pts), near, dev(v), dev(f), slot, max_dist=max_dist, history_row=hist, workspace=ws) is slot
    torch.cuda.synchronize()
    got, h = slot_of(slot), hist.cpu().numpy()
    assert same_bits(ws_part(ws, "step", 29), ref["sums"])
    assert (got["used"], got["skipped"], got["trimmed"], got["status"]) == (ref["used"], ref["skipped"], ref["trimmed"], ref["status"]) and ref["status"] == ac.OK
    assert (h[1], h[2], h[3]) == (ref["used"], ref["trimmed"], ref["status"]) and same_bits(h[0], got["rms"])
    assert abs(got["rms"] - ref["rms"]) <= TOL and got["wsum"] == ref["used"]
    assert np.linalg.cond(ref["A"]) <= 1e3
    print(f"align_step max_dist {max_dist}: {differing(got['M'], ref['M'])} of 12 entries of M differ from the restatement in their bits; "
          f"cond {np.linalg.cond(ref['A']):.3g}")
    assert np.abs(got["M"] - ref["M"]).max() <= TOL
    assert got["scale"] == 1.0 and same_bits(got["pivot"], pivot)


def test_align_step_few_pairs_and_the_sphere():
    pts, closest, face, dist, v, f = step_case()
    slot = F.align_init(dev(pts))
    before = slot.cpu().numpy().copy()
    near = {"closest": dev(closest[:5]), "face": dev(face[:5]), "dist": dev(dist[:5])}
    F.align_step(dev(pts[:5]), near, dev(v), dev(f), slot)
    got = slot_of(slot)
    assert got["status"] == ac.FEW and got["used"] == 1 and got["skipped"] == 4 and np.array_equal(got["M"], ac.IDENTITY)
    assert same_bits(got["pivot"], before[L.XFORM_PIVOT:L.XFORM_PIVOT + 3])
    empty = {"closest": torch.empty((0, 3), device=DEV), "face": torch.empty((0,), device=DEV, dtype=torch.int32), "dist": torch.empty((0,), device=DEV)}
    F.align_step(torch.empty((0, 3), device=DEV), empty, dev(v), dev(f), slot)
    got = slot_of(slot)
    assert got["status"] == ac.FEW and got["used"] == 0 and np.isnan(got["rms"]) and np.array_equal(got["M"], ac.IDENTITY)
    # a sphere has no rotation to find: singular, or a finite step
    sv, sf = mm.icosphere(2)
    sp = ac.surface_samples(sv, sf, 500, seed=1) * np.float32(1.01)
    c, fa, d = ac.correspondences(sp, sv, sf)
    slot = F.align_init(dev(sp))
    F.align_step(dev(sp), {"closest": dev(c), "face": dev(fa), "dist": dev(d)}, dev(sv), dev(sf), slot)
    got, ref = slot_of(slot), ac.align_step(sp, c, fa, d, sv, sf, INF, ac.IDENTITY, ac.pivot_of(sp))
    assert got["status"] == ref["status"] and got["status"] in (ac.OK, ac.SINGULAR)
    assert np.isfinite(got["M"]).all() and np.isfinite(got["rms"]) and got["used"] == 500


# ---------------------------------------------------------------- align_mesh

def check_history(history):
    assert (history[:, 3] == ac.OK).all()
    assert history[-1, 0] < 1e-5
    small = int(np.argmax(history[:, 0] < 1e-5))
    assert (np.diff(history[1:small + 1, 0]) <= 0).all(), history[:, 0]


@pytest.mark.parametrize("name", sorted(ac.MISPLACEMENTS))
def test_align_mesh_recovers_the_misplacement(name):
    """mesh onto mesh: the off-centre ellipsoid, misplaced, registered onto itself"""
    v, f = ac.ellipsoid(ac.OFF_CENTRE)
    A, truth = ac.misplacement(name, ac.OFF_CENTRE)
    moved = mm.f32(ac.apply(A, v.astype(np.float64)))
    res = F.align_mesh((moved, f), (v, f), iterations=10, n_samples=2000, seed=3, device=DEV)
    t, history = F.read_transform(res["transform"]), res["history"].cpu().numpy()
    check_history(history)
    assert (history[:, 1] == 2000).all() and t["status"] == "ok" and t["used"] == 2000 and t["scale"] == 1.0
    samples = F.sample_surface(dev(moved), dev(f), 2000, seed=3)["points"].cpu().numpy().astype(np.float64)
    err = np.abs(ac.apply(t["matrix"][:3], samples) - ac.apply(truth, samples)).max()
    print(f"align_mesh {name}: max error {err:.3g} (bound {ac.loop_bound(samples):.3g}); rms per iteration {history[:, 0]}")
    assert err <= ac.loop_bound(samples)
    assert abs(t["rotation_deg"] - ac.MISPLACEMENTS[name][1]) < 1e-3


def test_align_mesh_trims_the_outliers_and_follows_the_restatement():
    """the host test's trimming case on its own points: every tenth one is 3 away on each axis, max_dist 0.3"""
    pts, (v, f), truth = ac.icp_case("15deg", outliers=True)
    res = F.align_mesh(None, (v, f), iterations=10, max_dist=0.3, points=dev(pts))
    t, history = F.read_transform(res["transform"]), res["history"].cpu().numpy()
    check_history(history)
    assert (history[:, 1] == 900).all() and (history[:, 2] == 100).all() and t["used"] == 900 and t["trimmed"] == 100
    inlier = np.arange(len(pts)) % 10 != 0
    err = np.abs(ac.apply(t["matrix"][:3], pts[inlier]) - ac.apply(truth, pts[inlier])).max()
    print(f"align_mesh trimmed: max error {err:.3g} (bound {ac.loop_bound(pts[inlier]):.3g})")
    assert err <= ac.loop_bound(pts[inlier])
    # a starting matrix is honoured: from the true transform the first residual is already at the float32 floor
    start = F.align_mesh(None, (v, f), iterations=1, max_dist=0.3, points=dev(pts), init=np.vstack([truth, [0, 0, 0, 1]]))
    assert start["history"].cpu().numpy()[0, 0] < 1e-5


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    pts, (v, f), _ = ac.icp_case("30deg", outliers=True)
    tp, tv, tf = dev(pts), dev(v), dev(f)
    run = lambda: F.align_mesh(None, (tv, tf), iterations=6, max_dist=0.3, points=tp)
    outs = lambda r: [r["transform"].cpu().numpy().tobytes(), r["history"].cpu().numpy().tobytes()]
    first = outs(run())                                     # (also loads the kernels before the capture)
    assert outs(run()) == first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = run()
    for _ in range(2):
        res["transform"].fill_(7.0)                          # both are written by the calls
        res["history"].fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert outs(res) == first


def test_an_overflowed_grid_is_reported_at_the_read():
    v, f = ac.ellipsoid()
    res = F.align_mesh((v, f), (v, f), iterations=2, n_samples=500, entry_cap=16, device=DEV)
    h = res["history"].cpu().numpy()
    assert (h[:, 3] == ac.FEW).all() and (h[:, 1] == 0).all()
    with pytest.raises(L.GpnerfError, match="entry_cap"):
        F.read_transform(res["transform"])


# ---------------------------------------------------------------- mesh_metrics(align="rigid") and the evaluator

def test_mesh_metrics_after_registration():
    """the ellipsoid rotated 5 degrees and shifted 0.05 against itself: the offset decides the numbers until it is registered away"""
    v, f = ac.ellipsoid()
    R = ac.rotation((1.0, 1.0, 0.5), 5.0)
    pred = mm.f32(v.astype(np.float64) @ R.T + [0.05, 0.0, 0.0])
    th = (0.005, 0.01, 0.02)
    # the unaligned numbers on the host restatement first
    d_host = mm.nearest(ac.surface_samples(pred, f, 1000, seed=0), v, f)[0]
    assert d_host.mean() > 1.2e-2 and (d_host <= 0.005).mean() < 0.4
    plain = F.mesh_metrics((pred, f), (v, f), n_samples=4000, thresholds=th, device=DEV)
    none = F.mesh_metrics((pred, f), (v, f), n_samples=4000, thresholds=th, device=DEV, align=None)
    assert plain.cpu().numpy().tobytes() == none.cpu().numpy().tobytes()
    slots, transform = F.mesh_metrics((pred, f), (v, f), n_samples=4000, thresholds=th, device=DEV, align="rigid", want_transform=True)
    before, after, t = F.read_mesh_metrics(plain, th), F.read_mesh_metrics(slots, th), F.read_transform(transform)
    print(f"accuracy {before['accuracy']:.3g} -> {after['accuracy']:.3g}; precision@0.005 {before['precision@0.005']:.3g} -> "
          f"{after['precision@0.005']:.3g}; rotation {t['rotation_deg']:.4f} deg, rms {t['rms']:.3g}")
    assert before["accuracy"] > 1e-2 and before["precision@0.005"] < 0.5
    assert after["accuracy"] < 1e-4 and after["precision@0.005"] == 1.0 and after["completeness"] < 1e-4
    assert t["status"] == "ok" and abs(t["rotation_deg"] - 5.0) < 1e-2
    assert F.mesh_metrics((pred, f), (v, f), n_samples=4000, thresholds=th, device=DEV, want_transform=True)[1] is None


def _frames():
    axes = [np.linspace(-0.2, 0.2, 9).astype(np.float32), np.linspace(0.0, 0.5, 11).astype(np.float32), np.linspace(-0.1, 0.1, 5).astype(np.float32)]
    rng = np.random.default_rng(4)
    out = []
    for i in range(2):
        cube = np.pad(rng.uniform(0, 0.04, (9, 11, 5)).astype(np.float32), 10)
        v, f = ac.ellipsoid()
        pred = M.Mesh(mm.f32(v * 3.0 + [14, 15, 12]), f)      # index units of the padded cube
        gt = pred.to_lattice_frame(axes, 10)
        gt = M.Mesh(mm.f32(gt.vertices + [0.004 * (i + 1), 0.0, -0.003]), gt.faces)
        out.append(({"cube": cube, "mesh": pred, "axes": axes}, {"frame_index": torch.tensor([i]), "gt_mesh": gt}))
    return out


def test_mesh_evaluator_with_registration(tmp_path):
    frames = _frames()
    e = ev.MeshEvaluator(str(tmp_path / "a"), 0.02, metric_samples=4000, align="rigid")
    off = ev.MeshEvaluator(str(tmp_path / "b"), 0.02, metric_samples=4000)
    for output, batch in frames:
        e.evaluate(output, batch)
        off.evaluate(output, batch)
    s, s_off = e.summarize(), off.summarize()
    per, per_off = s.pop("per_frame"), s_off.pop("per_frame")
    new = {"align_rms", "align_rotation_deg", "align_translation", "align_status"}
    assert set(per) - set(per_off) == new and set(s) - set(s_off) == new - {"align_status"} and not new & set(per_off)
    assert per["align_status"] == [0, 0] and per["frame_index"] == [0, 1]
    for i in range(2):
        shift = np.linalg.norm([0.004 * (i + 1), 0.0, -0.003])
        assert abs(per["align_translation"][i] - shift) < 1e-4 and per["align_rotation_deg"][i] < 0.05 and per["align_rms"][i] < 1e-5
        assert per_off["accuracy"][i] > 1e-3 and per["accuracy"][i] < 1e-5
    moves = np.load(tmp_path / "a" / "align_transforms.npy")
    assert moves.shape == (2, 4, 4) and np.array_equal(moves[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (2, 1)))
    assert np.abs(moves[1, :3, 3] - [0.008, 0.0, -0.003]).max() < 1e-4
    assert sorted(os.listdir(tmp_path / "a")) == ["align_transforms.npy", "mesh_metrics.npy", "pts"]
    assert sorted(os.listdir(tmp_path / "b")) == ["mesh_metrics.npy", "pts"]
    assert e.summarize() == {}
    with pytest.raises(L.GpnerfError):
        ev.MeshEvaluator(str(tmp_path), 0.02, align="affine")
