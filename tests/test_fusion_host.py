"""CPU: the depth-fusion restatement (tests/fusion_cases.py) against what the definition promises -- every fate reached, every comparison
at its edge, the analytic sphere's zero set, a convex mesh's signs --, and the refusals of the gpnerf_fusion_* entry points and their
Python wrappers, none of which needs a device."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

import fusion_cases as fc


def test_the_general_case_reaches_every_fate():
    g = fc.general_case()
    assert g["dims"] == (20, 17, 65) and g["depth"].shape == (8, 20, 24)
    d, w = g["depth"], g["weights"]
    assert np.isnan(d).any() and (d == 0).any() and (d < 0).any() and np.isposinf(d).any() and np.isneginf(d).any()
    assert (w == 0).any() and np.isnan(w).any()
    n = int(np.prod(g["dims"]))
    for carve in (True, False):
        ref = fc.run_case(g, carve=carve)
        per_fate = dict(zip(fc.FATES, ref["stats"].sum(axis=0).tolist()))
        print(f"general case, carve={carve}: {n} points x 8 views; pairs per fate {per_fate}; totals {dict(zip(fc.TOTALS, ref['totals'].tolist()))}")
        assert all(c >= 1 for c in per_fate.values()), per_fate
        assert (ref["stats"].sum(axis=1) == n).all(), "a view's row sums to the number of lattice points"
        t = ref["totals"]
        assert t[0] + t[2] + t[3] == n and min(t) >= 1
        assert np.abs(ref["values"]).max() <= np.float32(g["band"]) and np.isfinite(ref["values"]).all()
    plain = fc.run_case(g, weights=None)
    assert not np.array_equal(plain["values"], fc.run_case(g)["values"]), "the weights matter"


def test_every_comparison_at_its_edge():
    for name, case in fc.boundary_cases().items():
        ref = fc.run_case(case)
        assert np.array_equal(ref["fate"], case["expect"]), (name, ref["fate"].tolist(), case["expect"].tolist())
        if "values" in case:
            assert np.array_equal(ref["values"], case["values"]), name
    c = fc.boundary_cases()
    tiny = fc.run_case(c["weights_tiny_alone"])
    assert tiny["values"].ravel().tolist() == [0.125] and tiny["totals"].tolist() == [1, 1, 0, 0], "a weight of 1e-30 weighs in"
    hidden = fc.run_case(dict(c["depth"], depth=c["depth"]["depth"][1:2], Ks=c["depth"]["Ks"][:1], RTs=c["depth"]["RTs"][:1]))
    assert hidden["values"].ravel().tolist() == [-0.25] and hidden["flags"].ravel().tolist() == [fc.FLAG_HIDDEN]
    assert hidden["totals"].tolist() == [0, 0, 1, 0], "unseen and hidden: interior"
    nodata = fc.run_case(dict(c["depth"], depth=c["depth"]["depth"][4:5], Ks=c["depth"]["Ks"][:1], RTs=c["depth"]["RTs"][:1]))
    assert nodata["values"].ravel().tolist() == [0.25] and nodata["totals"].tolist() == [0, 0, 0, 1], "unknown reads as empty"


def test_chunks_of_views_leave_the_same_bits():
    g = fc.general_case(dims=(12, 10, 9))
    whole = fc.run_case(g)
    for chunks in ([range(0, 4), range(4, 8)], [[v] for v in range(8)]):
        part = fc.run_case(g, chunks=chunks)
        for k in ("values", "flags", "sum", "weight", "stats", "totals"):
            assert np.array_equal(whole[k].view(np.uint8), part[k].view(np.uint8)), k


def test_the_analytic_spheres_zero_set():
    """Six axis views of the unit sphere, nearest-pixel depth.  WHAT CAN BE DERIVED of the projective distance is the sign away from the
    surface, not the crossing's place.  A pair (p, view) that is not BEHIND / OUTSIDE / NODATA reads the depth d' of the ray through
    a pixel centre at most half a pixel's diagonal from p's projection; that ray's point q at p's camera depth z lies in the plane of
    constant z, |q - p| <= z / focal * sqrt(1/2) =: footprint.
      - p INSIDE, deeper than the footprint: q is inside too, so the ray has met the sphere in front of q: d' < z, s < 0, the pair is
        NEAR with t < 0 or HIDDEN.  No pair gives such a point a t >= 0: its value is negative (or -band, interior-filled).
      - p OUTSIDE and a pair with s < 0: the ray entered the sphere in front of q and, q being outside a convex body, left it again: q
        lies beyond the chord.  If the pair is not HIDDEN, the entry lies within band of q in camera z, band * |direction| <= band *
        d_max along the ray.  With h <= r the line's distance from the centre and a <= band d_max q's distance from the chord's
        middle, |q|^2 = h^2 + a^2 <= r^2 + (band d_max)^2: q lies within graze = sqrt(r^2 + (band d_max)^2) - r of the sphere, p
        within graze + footprint.  Farther out every contributing pair has t > 0.
      - every outside lattice point has a contributing pair: the camera on the axis of its largest |coordinate| sees it in front of
        the sphere's tangent plane there, and the images cover the lattice (asserted).
    So: value < 0 at inside points deeper than slack_in, value > 0 at outside points farther than slack_out -- asserted at ALL such
    points.  A zero crossing on a lattice edge (a, b) then has an end that is not far outside and one that is not deep inside; the
    distance to the sphere g = |.| - r is convex and 1-Lipschitz, so on the edge -slack_in - step <= g <= slack_out + step: asserted.
    That the crossings found lie under ONE step is printed and asserted as measured on the restatement: the issue's bound."""
    s = fc.sphere_case()
    ref = fc.run_case(s)
    assert ref["stats"][:, fc.OUTSIDE].sum() == 0 and ref["stats"][:, fc.BEHIND].sum() == 0, "the images cover the lattice"
    p = fc.lattice_points(s["lo"], s["step"], s["dims"]).astype(np.float64)
    g = np.linalg.norm(p, axis=1) - s["radius"]
    v = ref["values"].ravel()
    step = float(s["step"][0])
    deep, far = g < -s["slack_in"], g > s["slack_out"]
    print(f"sphere: {len(p)} points, step {step}, band {s['band']}, footprint {s['footprint']:.4f}, slack in {s['slack_in']:.4f} out "
          f"{s['slack_out']:.4f}; {int(deep.sum())} deep inside, {int(far.sum())} far outside, {int((~deep & ~far).sum())} undecided")
    assert s["slack_out"] < step and deep.sum() > 2000 and far.sum() > 10000
    assert (v[deep] < 0).all() and (v[far] > 0).all()
    wrong = ((v <= 0) != (g <= 0)) & ~deep & ~far
    print(f"sphere: {int(wrong.sum())} of the undecided points carry the other sign than the sphere's")
    # offset_mesh(0)'s crossings: marching cubes takes value <= 0 as inside and interpolates linearly along an edge
    V = ref["values"].astype(np.float64)
    P = p.reshape(s["dims"] + (3,))
    worst = 0.0
    count = 0
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        va, vb, pa, pb = V[tuple(a)], V[tuple(b)], P[tuple(a)], P[tuple(b)]
        cross = (va <= 0) != (vb <= 0)
        t = (0.0 - va[cross]) / (vb[cross] - va[cross])
        c = pa[cross] + t[:, None] * (pb[cross] - pa[cross])
        worst = max(worst, float(np.abs(np.linalg.norm(c, axis=1) - s["radius"]).max()))
        count += int(cross.sum())
    print(f"sphere: {count} zero crossings on lattice edges, max distance to the sphere {worst:.4f} = {worst / step:.3f} steps")
    assert count > 1000
    assert worst < step + s["slack_out"], "the derived bound"
    assert worst < step, "the issue's bound: under one lattice step"


def test_a_convex_meshs_signs_on_the_restatement_alone():
    """The case of the GPU test beside mesh_sdf, on the host: depth maps by the restated ray cast, the sign of the restated field against
    the polyhedron's inside / outside wherever the distance to it exceeds the margin.  |p| > 1 + margin is outside and farther than the
    margin from it (the vertices lie on the unit sphere); |p| < r_in - margin is inside and deeper than it.  margin = footprint + one
    lattice step: the sphere argument of test_the_analytic_spheres_zero_set holds for a convex polyhedron between two spheres with
    graze = sqrt(1 + 2 c0 b + b^2) - r_in, b = band d_max, c0 = sqrt(1 - r_in^2) (the chord's middle is within c0 of the polyhedron's
    own chord), which must stay under the one lattice step -- asserted."""
    m = fc.convex_case()
    b = m["band"] * m["d_max"]
    graze = np.sqrt(1.0 + 2.0 * np.sqrt(1.0 - m["r_in"] ** 2) * b + b * b) - m["r_in"]
    step = float(m["step"][0])
    print(f"convex: r_in {m['r_in']:.5f}, footprint {m['footprint']:.4f}, graze {graze:.4f}, margin {m['margin']:.4f}")
    assert graze < step
    ref = fc.run_case(dict(m, depth=fc.mesh_depth(m)))
    assert ref["stats"][:, fc.OUTSIDE].sum() == 0 and ref["stats"][:, fc.BEHIND].sum() == 0
    r = np.linalg.norm(fc.lattice_points(m["lo"], m["step"], m["dims"]).astype(np.float64), axis=1)
    v = ref["values"].ravel()
    inside, outside = r < m["r_in"] - m["margin"], r > 1.0 + m["margin"]
    share = 1.0 - (inside.sum() + outside.sum()) / len(r)
    print(f"convex: {len(r)} points, {int(inside.sum())} inside and {int(outside.sum())} outside compared, {share:.3f} left out (cap {m['cap']:.3f})")
    assert share < m["cap"]
    assert (v[inside] < 0).all() and (v[outside] > 0).all()


def test_fusion_entry_points_refuse_bad_arguments_on_the_host(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    P = 0x1000
    cams = np.ascontiguousarray(np.tile(np.concatenate([fc.EXACT_K.ravel(), fc.EXACT_RT.ravel()]), 8), np.float64)
    lat = np.array([0, 0, 0, 0.5, 0.25, 1.0], np.float64)
    dims = (C.c_int32 * 3)(4, 5, 6)
    nan, inf = float("nan"), float("inf")

    def call(entry, depth=P, weights=None, cams=cams, views=2, H=8, W=8, lat=lat, dims=dims, band=0.5, z_near=1e-6, carve=1, sum_=P, weight=P,
             flags=P, sdf=P, stats=P, totals=P):
        cp = None if cams is None else cams.ctypes.data_as(L.DP)
        lp = None if lat is None else np.ascontiguousarray(lat, np.float64).ctypes.data_as(L.DP)
        if entry == "integrate":
            return lib.gpnerf_fusion_integrate(depth, weights, cp, views, H, W, lp, dims, band, z_near, carve, sum_, weight, flags, stats, None)
        return lib.gpnerf_fusion_oneshot(depth, weights, cp, views, H, W, lp, dims, band, z_near, carve, sdf, flags, stats, totals, None)

    bad_lat = lambda i, v: np.concatenate([lat[:i], [v], lat[i + 1:]])
    shared = [dict(depth=None), dict(cams=None), dict(lat=None), dict(dims=None), dict(stats=None), dict(views=0), dict(views=9), dict(H=0),
              dict(W=0), dict(H=16385), dict(W=16385), dict(band=0.0), dict(band=-1.0), dict(band=nan), dict(band=inf),
              dict(band=0.25 * 1024 * 1.001), dict(z_near=0.0), dict(z_near=-1.0), dict(z_near=nan), dict(z_near=inf), dict(carve=2),
              dict(carve=-1), dict(dims=(C.c_int32 * 3)(0, 5, 6)), dict(dims=(C.c_int32 * 3)(4, 5, -1)),
              dict(dims=(C.c_int32 * 3)(1 << 14, 1 << 14, 2)), dict(dims=(C.c_int32 * 3)(1 << 15, 1 << 15, 1)), dict(lat=bad_lat(0, nan)),
              dict(lat=bad_lat(1, inf)), dict(lat=bad_lat(3, 0.0)), dict(lat=bad_lat(4, -0.25)), dict(lat=bad_lat(5, nan)),
              dict(lat=bad_lat(5, inf))]
    for kw in shared + [dict(sum_=None), dict(weight=None), dict(flags=None)]:
        assert call("integrate", **kw) == -1, ("integrate", kw)
    for kw in shared + [dict(sdf=None), dict(totals=None)]:
        assert call("oneshot", **kw) == -1, ("oneshot", kw)
    for args in ((None, P, P, P), (dims, None, P, P), (dims, P, None, P), (dims, P, P, None), ((C.c_int32 * 3)(0, 1, 1), P, P, P),
                 ((C.c_int32 * 3)(1 << 14, 1 << 14, 2), P, P, P)):
        assert lib.gpnerf_fusion_reset(*args, None) == -1, args
    fin = lambda sum_=P, weight=P, flags=P, dims=dims, band=0.5, sdf=P, totals=P: lib.gpnerf_fusion_finalise(sum_, weight, flags, dims, band, sdf,
                                                                                                           totals, None)
    for kw in (dict(sum_=None), dict(weight=None), dict(flags=None), dict(dims=None), dict(sdf=None), dict(totals=None), dict(band=0.0),
               dict(band=-1.0), dict(band=nan), dict(band=inf), dict(dims=(C.c_int32 * 3)(4, 0, 6))):
        assert fin(**kw) == -1, kw
    hdr = open(os.path.join(os.path.dirname(pkg.__file__), "..", "include", "gpnerf_hip.h")).read()
    for i, name in enumerate(L.FUSION_FATES):
        assert f"#define GPNERF_FUSION_{name.upper()} {i}\n" in hdr, name
        assert getattr(L, f"FUSION_{name.upper()}") == i and fc.FATES[i] == name
    for i, name in enumerate(L.FUSION_TOTALS):
        assert f"#define GPNERF_FUSION_{name.upper()} {i}\n" in hdr, name
        assert getattr(L, f"FUSION_{name.upper()}") == i and fc.TOTALS[i] == name
    assert f"#define GPNERF_FUSION_FATES {L.FUSION_N_FATES}\n" in hdr and L.FUSION_N_FATES == len(L.FUSION_FATES)
    assert f"#define GPNERF_FUSION_TOTALS {L.FUSION_N_TOTALS}\n" in hdr and L.FUSION_N_TOTALS == len(L.FUSION_TOTALS)
    assert f"#define GPNERF_FUSION_FLAG_HIDDEN {L.FUSION_FLAG_HIDDEN}\n" in hdr and L.FUSION_FLAG_HIDDEN == fc.FLAG_HIDDEN
    assert f"#define GPNERF_FUSION_FLAG_NEAR {L.FUSION_FLAG_NEAR}\n" in hdr and L.FUSION_FLAG_NEAR == fc.FLAG_NEAR
    assert f"#define GPNERF_FUSION_MAX_VIEWS {L.FUSION_MAX_VIEWS}\n" in hdr


def test_the_wrappers_refuse_cpu_tensors_and_bad_options(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    K, RT = fc.EXACT_K[None], fc.EXACT_RT[None]
    lattice = dict(lo=(0, 0, 0), step=(0.5, 0.5, 0.5), dims=(3, 3, 3))
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.fuse_depth(torch.ones(1, 9, 9), K, RT, band=1.0, **lattice)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.DepthFusion(band=1.0, device="cpu", **lattice)
    with pytest.raises(pkg.GpnerfError, match="depth must be a device tensor"):
        F.fuse_depth(np.ones((1, 9, 9), np.float32), K, RT, band=1.0, **lattice)
    with pytest.raises(pkg.GpnerfError, match="band .* refused"):
        F.fuse_depth(torch.ones(1, 9, 9), K, RT, band=0.5 * 1025, **lattice)
    with pytest.raises(pkg.GpnerfError, match="band .* refused"):
        F.DepthFusion(band=float("nan"), device="cuda:0", **lattice)
    with pytest.raises(pkg.GpnerfError, match="dims"):
        F.fuse_depth(torch.ones(1, 9, 9), K, RT, band=1.0, lo=(0, 0, 0), step=(1, 1, 1), dims=(0, 3, 3))


def test_read_fusion_stats_names_and_fractions(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    stats = np.array([[1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1]], np.int64)
    r = F.read_fusion_stats(stats, np.array([12, 7, 3, 6], np.int64))
    assert set(r["per_view"]) == set(pkg._lib.FUSION_FATES) and r["per_view"]["near"] == [6, 1] and r["per_view"]["behind"] == [1, 6]
    assert (r["seen"], r["surface"], r["interior"], r["unknown"]) == (12, 7, 3, 6) and r["seen_fraction"] == 12 / 21
    assert F.read_fusion_stats(np.zeros((1, 6)), np.zeros(4))["seen_fraction"] == 0.0
