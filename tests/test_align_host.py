"""CPU: the numpy restatement of the registration entry points (tests/align_cases.py) against numpy.linalg and against the transform
it has to recover, and the host side of the C entry points (refusals, the workspace's size, the constants)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import align_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rotation_angle(R):
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("with_scale", [False, True])
def test_the_closed_form_agrees_with_svd(seed, with_scale):
    """R, t, s of the restated Jacobi / Horn solve within 1e-13 of SVD-Kabsch / Umeyama, on weighted sets whose top eigenvalue gap is
    at least 0.1 of the largest and whose source scatter has cond <= 1e3 (the GPU test's 2^-32 argument relies on it)."""
    src, dst, w = ac.pair_set(500, seed, weights=True, scale=1.7 if with_scale else 1.0)
    gap, cond = ac.eigen_gap(src, dst, w)
    assert gap >= 0.1 and cond <= 1e3, (gap, cond)
    r = ac.rigid_fit(src, dst, w, with_scale)
    R, t, s = ac.kabsch(src, dst, w, with_scale)
    assert r["status"] == ac.OK and r["used"] == 500
    print(f"seed {seed} scale {with_scale}: gap {gap:.3g} cond {cond:.3g} dR {np.abs(r['M'][:, :3] - s * R).max():.3g} "
          f"dt {np.abs(r['M'][:, 3] - t).max():.3g} ds {abs(r['scale'] - s):.3g}")
    assert np.abs(r["M"][:, :3] - s * R).max() <= 1e-13
    assert np.abs(r["M"][:, 3] - t).max() <= 1e-13
    assert abs(r["scale"] - s) <= 1e-13


def test_the_dirty_pairs_are_skipped_and_the_rest_is_fit():
    src, dst, w = ac.pair_set(700, 11, dirty=True)
    r = ac.rigid_fit(src, dst, w)
    ok = np.isfinite(src).all(1) & np.isfinite(dst).all(1) & np.isfinite(w) & (w > 0)
    assert 0 < ok.sum() < 700 and r["used"] == ok.sum() and r["skipped"] == 700 - ok.sum()
    R, t, _ = ac.kabsch(src, dst, w)
    assert np.abs(r["M"][:, :3] - R).max() <= 1e-13 and np.abs(r["M"][:, 3] - t).max() <= 1e-13


def test_coplanar_pairs_are_still_well_defined():
    """Horn's quaternion needs no third dimension: a planar set, rotated rigidly, is recovered (SVD needs its reflection fix there)"""
    rng = np.random.default_rng(5)
    src = np.concatenate([rng.normal(size=(300, 2)), np.zeros((300, 1))], axis=1)
    R = ac.rotation((1, 2, 3), 40.0)
    dst = src @ R.T + np.array([0.3, -0.2, 0.5])
    r = ac.rigid_fit(src, dst)
    Rk, tk, _ = ac.kabsch(src, dst)
    assert r["status"] == ac.OK
    assert np.abs(r["M"][:, :3] - Rk).max() <= 1e-13 and np.abs(r["M"][:, 3] - tk).max() <= 1e-13
    assert abs(np.linalg.det(r["M"][:, :3]) - 1) < 1e-12


@pytest.mark.parametrize("n", [0, 1, 2])
def test_too_few_pairs(n):
    src, dst, _ = ac.pair_set(n, 1)
    r = ac.rigid_fit(src, dst)
    assert r["status"] == ac.FEW and r["used"] == n and np.array_equal(r["M"], ac.IDENTITY)


def test_equal_points_are_singular():
    src = np.tile(np.float32([[1, 2, 3]]), (50, 1))
    dst, _, _ = ac.pair_set(50, 2)
    assert ac.rigid_fit(src, dst)["status"] == ac.SINGULAR                   # sum w |a|^2 == 0
    r = ac.rigid_fit(dst, src)                                               # S == 0: the four eigenvalues are equal
    assert r["status"] == ac.SINGULAR and np.array_equal(r["M"], ac.IDENTITY) and np.isfinite(r["rms"])


def test_the_strided_tree_sum_is_a_sum():
    rng = np.random.default_rng(0)
    for n in (0, 1, 255, 257, 16385, 40000):
        x = rng.normal(size=(n, 3))
        assert np.allclose(ac.strided_tree_sum(x), x.sum(axis=0), rtol=0, atol=1e-9)
    ints = rng.integers(-1000, 1000, size=(40000, 2)).astype(np.float64)
    assert np.array_equal(ac.strided_tree_sum(ints), ints.sum(axis=0))       # exact terms: exact in any order


def test_the_cholesky_solve_against_numpy():
    rng = np.random.default_rng(3)
    for _ in range(10):
        B = rng.normal(size=(40, 6)) * rng.uniform(0.1, 3.0, 6)
        A, g = B.T @ B, rng.normal(size=6)
        status, x = ac.cholesky_solve6(A, g)
        assert status == ac.OK
        ref = np.linalg.solve(A, g)
        assert np.abs(np.array(x) - ref).max() <= 1e-12 * np.linalg.cond(A) * np.abs(ref).max()
    B = rng.normal(size=(40, 6))
    B[:, 5] = B[:, 0] + B[:, 1]                                             # rank 5
    assert ac.cholesky_solve6(B.T @ B, np.ones(6))[0] == ac.SINGULAR
    assert ac.cholesky_solve6(np.zeros((6, 6)), np.ones(6))[0] == ac.SINGULAR


def test_the_cayley_update_is_a_rigid_motion_about_the_pivot_image():
    M = np.hstack([ac.rotation((0, 1, 1), 20.0), [[1.0], [2.0], [3.0]]])
    pivot = np.array([10.0, -5.0, 3.0])
    x = [0.02, -0.01, 0.03, 0.1, 0.2, -0.3]
    Mn = ac.step_update(M, pivot, x)
    assert np.abs(Mn[:, :3] @ Mn[:, :3].T - np.eye(3)).max() < 1e-15 * 8
    cp = np.array(ac.pivot_image(M, pivot))
    assert np.abs(ac.apply(Mn, pivot) - (cp + x[3:])).max() < 1e-14        # the pivot's image moves by u alone
    step = Mn[:, :3] @ M[:, :3].T
    assert abs(rotation_angle(step) - 2 * np.arctan(np.linalg.norm(x[:3]) / 2)) < 1e-15 * 8
    assert np.array_equal(ac.step_update(M, pivot, [0.0] * 6), M)           # a zero step is the identity, bit for bit


@functools.lru_cache(maxsize=None)
def loop(name, outliers=False):
    pts, (v, f), truth = ac.icp_case(name, outliers=outliers)
    M, history, pivot = ac.icp(pts, v, f, iterations=10, max_dist=0.3 if outliers else np.inf)
    return pts, (v, f), truth, M, history


@pytest.mark.parametrize("name", sorted(ac.MISPLACEMENTS))
def test_the_loop_recovers_the_misplacement(name):
    """1 000 float32 surface samples of the off-centre ellipsoid, rotated 15 / 30 degrees about its centre and shifted 0.1 / 0.2, driven
    by mesh_metric_cases.nearest in float32: after 10 iterations max |M p - M_true p| <= 2^-18 max |coordinate|."""
    pts, _, truth, M, history = loop(name)
    err = np.abs(ac.apply(M, pts) - ac.apply(truth, pts)).max()
    print(f"{name}: max error {err:.3g} (bound {ac.loop_bound(pts):.3g}); rms per iteration {history[:, 0]}")
    assert (history[:, 3] == ac.OK).all() and (history[:, 1] == 1000).all()
    assert err <= ac.loop_bound(pts)
    assert history[-1, 0] < 1e-5
    first_small = np.argmax(history[:, 0] < 1e-5)
    assert (np.diff(history[1:first_small + 1, 0]) <= 0).all()


def test_the_loop_trims_the_outliers():
    """every tenth sample moved by +3 on each axis, max_dist 0.3: 900 pairs used from the first iteration on, the same bound"""
    pts, (v, f), truth, M, history = loop("15deg", outliers=True)
    inlier = np.arange(len(pts)) % 10 != 0
    d0 = ac.correspondences(pts, v, f)[2]
    assert (d0[inlier] <= 0.3).all() and (d0[~inlier] > 0.3).all()           # a condition on the input
    assert (history[:, 1] == 900).all() and (history[:, 2] == 100).all()
    err = np.abs(ac.apply(M, pts[inlier]) - ac.apply(truth, pts[inlier])).max()
    print(f"trimmed: max error {err:.3g} (bound {ac.loop_bound(pts[inlier]):.3g})")
    assert err <= ac.loop_bound(pts[inlier])


def test_the_plane_step_on_a_sphere_is_singular_or_finite():
    import mesh_metric_cases as mc
    v, f = mc.icosphere(2)
    pts = ac.surface_samples(v, f, 500, seed=1) * np.float32(1.01)
    closest, face, dist = ac.correspondences(pts, v, f)
    r = ac.align_step(pts, closest, face, dist, v, f, np.inf, ac.IDENTITY, ac.pivot_of(pts))
    assert r["status"] in (ac.OK, ac.SINGULAR) and np.isfinite(r["M"]).all()


# ---------------------------------------------------------------- the host side of the C entry points

def test_the_constants_are_the_headers(pkg):
    L = pkg._lib
    hdr = open(os.path.join(ROOT, "include", "gpnerf_hip.h")).read()
    define = lambda name: int(re.search(rf"#define GPNERF_{name} (\d+)\b", hdr).group(1))
    assert (L.ALIGN_THREADS, L.ALIGN_BLOCKS) == (define("ALIGN_THREADS"), define("ALIGN_BLOCKS")) == (ac.THREADS, ac.BLOCKS) == (256, 64)
    assert (L.ALIGN_OK, L.ALIGN_FEW, L.ALIGN_SINGULAR) == (define("ALIGN_OK"), define("ALIGN_FEW"), define("ALIGN_SINGULAR")) == (ac.OK, ac.FEW, ac.SINGULAR)
    for name in ("M", "SCALE", "STATUS", "USED", "SKIPPED", "TRIMMED", "WSUM", "RMS", "PIVOT", "DOUBLES"):
        assert getattr(L, f"XFORM_{name}") == define(f"XFORM_{name}"), name
    for name, at in L.ALIGN_WS.items():
        assert at == define(f"ALIGN_WS_{name.upper()}"), name
    assert L.ALIGN_WS_DOUBLES == define("ALIGN_WS_DOUBLES")
    assert L.XFORM_PIVOT + 3 <= L.XFORM_DOUBLES
    nbytes = L.lib().gpnerf_align_workspace_bytes()
    assert nbytes == 8 * L.ALIGN_WS_DOUBLES > 0
    assert L.ALIGN_WS["rows"] + L.ALIGN_BLOCKS * 29 <= L.ALIGN_WS["count_rows"] and L.ALIGN_WS["count_rows"] + 4 * L.ALIGN_BLOCKS <= L.ALIGN_WS_DOUBLES


def test_the_entry_points_refuse_bad_arguments_on_the_host(pkg):
    """GPNERF_E_ARG before any device call (the pointers are non-null dummies: a call that got past the checks would launch)"""
    lib = pkg._lib.lib()
    P, ws = 0x1000, int(lib.gpnerf_align_workspace_bytes())

    def fit(src=P, dst=P, w=None, n=10, slot=P, wsp=P, wsb=ws):
        return lib.gpnerf_rigid_fit(src, dst, w, n, 0, slot, wsp, wsb, None)

    for bad in (dict(src=None), dict(dst=None), dict(slot=None), dict(wsp=None), dict(n=-1), dict(wsb=ws - 1), dict(wsb=0)):
        assert fit(**bad) == -1, bad

    def init(points=P, n=10, m=None, slot=P, wsp=P, wsb=ws):
        return lib.gpnerf_align_init(points, n, m, slot, wsp, wsb, None)

    for bad in (dict(points=None), dict(slot=None), dict(wsp=None), dict(n=-1), dict(wsb=ws - 1),
                dict(m=(C.c_double * 12)(*([float("nan")] + [0.0] * 11))), dict(m=(C.c_double * 12)(*([0.0] * 12)))):
        assert init(**bad) == -1, bad

    def transform(points=P, n=10, slot=P, out=P):
        return lib.gpnerf_transform_points(points, n, slot, 0, out, None)

    for bad in (dict(points=None), dict(slot=None), dict(out=None), dict(n=-1)):
        assert transform(**bad) == -1, bad
    assert transform(n=0) == 0                                               # a no-op

    def step(cur=P, closest=P, face=P, dist=P, n=10, v=P, nv=8, f=P, nf=4, max_dist=1.0, slot=P, hist=None, wsp=P, wsb=ws):
        return lib.gpnerf_align_step(cur, closest, face, dist, n, v, nv, f, nf, max_dist, slot, hist, wsp, wsb, None)

    for bad in (dict(cur=None), dict(closest=None), dict(face=None), dict(dist=None), dict(v=None), dict(f=None), dict(slot=None),
                dict(wsp=None), dict(n=-1), dict(nv=-1), dict(nf=0), dict(wsb=ws - 1), dict(max_dist=0.0), dict(max_dist=-1.0),
                dict(max_dist=float("nan"))):
        assert step(**bad) == -1, bad


def test_cpu_tensors_are_refused(pkg):
    import importlib
    import torch
    fm = importlib.import_module("gp-nerf_amd.frame")
    p = torch.zeros(4, 3)
    slot = torch.zeros(pkg._lib.XFORM_DOUBLES, dtype=torch.float64)
    for call in (lambda: fm.rigid_fit(p, p), lambda: fm.transform_points(p, slot), lambda: fm.align_init(p),
                 lambda: fm.align_mesh(None, None, points=p)):
        with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
            call()
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        fm.align_mesh((np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32)), None, device="cpu")
    with pytest.raises(pkg.GpnerfError, match="align is None or 'rigid'"):
        fm.mesh_metrics(None, None, align="affine")
