"""CPU: the signed distance field's entry points refuse bad arguments on the host before anything is launched, the workspace formula,
the wrappers' refusals, and self-checks of the numpy restatements (tests/sdf_cases.py) the GPU tests compare against: the field on
analytic cases, the trilinear sampling against the eight-corner formula."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import mesh_metric_cases as mm
import sdf_cases as sc

P = 0x1000                                                   # a non-null dummy: argument checks never dereference


def _dims(*d):
    return (C.c_int32 * 3)(*d)


def test_mesh_sdf_rejects_bad_arguments_on_the_host(pkg):
    L = pkg._lib
    lib = L.lib()
    good_lat = np.array([0, 0, 0, 1, 0.5, 2], np.float64)
    big = 1 << 40

    def call(vertices=P, nv=10, faces=P, nf=5, lat=good_lat, dims=(12, 10, 9), band=1.5, bits=P, ws=P, ws_bytes=big, sdf=P, face_id=P, stats=P):
        lp = None if lat is None else np.ascontiguousarray(lat, np.float64).ctypes.data_as(L.DP)
        return lib.gpnerf_mesh_sdf(vertices, nv, faces, nf, lp, None if dims is None else _dims(*dims), band, bits, ws, ws_bytes, sdf, face_id,
                                   stats, None)

    lat = lambda i, v: np.concatenate([good_lat[:i], [v], good_lat[i + 1:]])
    # everything the voxeliser refuses of the arguments they share, a null sdf, and a bad band (the smallest step is 0.5: 512 at most)
    for bad in (dict(vertices=None), dict(faces=None), dict(lat=None), dict(dims=None), dict(ws=None), dict(sdf=None), dict(stats=None),
                dict(nv=-1), dict(nf=-1), dict(nf=1 << 31), dict(nv=1 << 31),
                dict(dims=(0, 10, 9)), dict(dims=(12, -1, 9)), dict(dims=(12, 10, 0)), dict(dims=(1 << 10, 1 << 10, (1 << 8) + 1)),
                dict(dims=(1 << 20, 1 << 20, 1)), dict(lat=lat(0, np.nan)), dict(lat=lat(2, np.inf)), dict(lat=lat(3, 0.0)),
                dict(lat=lat(4, -1.0)), dict(lat=lat(5, np.nan)), dict(lat=lat(5, np.inf)),
                dict(band=0.0), dict(band=-1.0), dict(band=float("nan")), dict(band=float("inf")), dict(band=512.5)):
        assert call(**bad) == -1, bad
    need = int(lib.gpnerf_mesh_sdf_workspace_bytes(5, _dims(12, 10, 9)))
    assert need > 0 and call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1


def test_sdf_sample_rejects_bad_arguments_on_the_host(pkg):
    L = pkg._lib
    lib = L.lib()
    lp = np.array([0, 0, 0, 1, 1, 1], np.float64).ctypes.data_as(L.DP)
    bad_step = np.array([0, 0, 0, 1, 0, 1], np.float64).ctypes.data_as(L.DP)

    def sample(sdf=P, dims=_dims(12, 10, 9), lat=lp, points=P, n=7, out=P):
        return lib.gpnerf_sdf_sample(sdf, dims, lat, points, n, out, None)

    for bad in (dict(sdf=None), dict(dims=None), dict(dims=_dims(12, 1, 9)), dict(dims=_dims(0, 4, 4)), dict(dims=_dims(1 << 10, 1 << 10, 1 << 9)),
                dict(lat=None), dict(lat=bad_step), dict(points=None), dict(out=None), dict(n=-1), dict(n=1 << 31)):
        assert sample(**bad) == -1, bad
    assert sample(points=None, out=None, n=0) == 0, "no points: nothing to launch"


def test_the_workspace_formula(pkg):
    """include/gpnerf_hip.h: 256 + align256(8 nx ny nz) + align256(4 n_faces): the header, a key per lattice point, a list entry per face
    at worst; host arithmetic only; 0 for what the call refuses"""
    lib = pkg._lib.lib()
    ws = lambda nf, d: int(lib.gpnerf_mesh_sdf_workspace_bytes(nf, _dims(*d)))
    al = lambda b: (b + 255) // 256 * 256
    for nf, d in ((0, (1, 1, 1)), (12, (12, 10, 9)), (12, (12, 10, 33)), (79948, (140, 90, 400)), (2 ** 31 - 1, (1 << 10, 1 << 10, 1 << 8)),
                  (7, (1, 1, 1 << 28))):
        assert ws(nf, d) == 256 + al(8 * d[0] * d[1] * d[2]) + al(4 * nf), (nf, d)
    for refused in ((-1, (4, 4, 4)), (1 << 31, (4, 4, 4)), (5, (0, 4, 4)), (5, (4, 4, -2)), (5, (1 << 10, 1 << 10, (1 << 8) + 1)),
                    (5, (1 << 16, 1 << 16, 1))):
        assert ws(*refused) == 0, refused
    assert int(lib.gpnerf_mesh_sdf_workspace_bytes(5, None)) == 0


def test_the_header_and_the_binding_name_the_same_constants(pkg):
    L = pkg._lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpnerf_hip.h")).read()
    value = lambda name: int(re.search(rf"#define GPNERF_SDF_{name} (\d+)\b", hdr).group(1))
    assert [value(n.upper()) for n in L.SDF_STATS] == list(range(8)) and value("STATS") == len(L.SDF_STATS) == len(sc.STATS)
    assert tuple(L.SDF_STATS) == sc.STATS
    assert value("LARGE_POINTS") == L.SDF_LARGE_POINTS == sc.LARGE_POINTS and value("MAX_BAND_STEPS") == L.SDF_MAX_BAND_STEPS == sc.MAX_BAND_STEPS


def test_the_wrappers_refuse_on_the_host(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    v, f = mm.one_triangle()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.mesh_sdf(tv, tf, (0, 0, 0), (1, 1, 1), (12, 10, 9), 1.5)
    for band in (0.0, -1.0, float("nan"), float("inf"), 1025.0):
        with pytest.raises(pkg.GpnerfError, match="band"):
            F.mesh_sdf(tv, tf, (0, 0, 0), (1, 1, 1), (12, 10, 9), band)
    with pytest.raises(pkg.GpnerfError, match="dims"):
        F.mesh_sdf(tv, tf, (0, 0, 0), (1, 1, 1), (12, 0, 9), 1.5)
    with pytest.raises(pkg.GpnerfError, match="step"):
        F.mesh_sdf(tv, tf, (0, 0, 0), (1, 0, 1), (12, 10, 9), 1.5)
    grid = F.SdfGrid(torch.zeros((4, 4, 4)), None, None, (0, 0, 0), (1, 1, 1), (4, 4, 4), 0.5, None)
    # offset_mesh refuses |offset| >= band before it touches the field
    for offset in (0.5, -0.5, 0.75, float("nan"), float("inf")):
        with pytest.raises(pkg.GpnerfError, match="band"):
            grid.offset_mesh(offset)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        grid.offset_mesh(0.25)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        grid.sample(torch.zeros((3, 3)))
    ev = importlib.import_module("gp-nerf_amd.evaluator")
    for band in (0, -2, 1025):
        with pytest.raises(pkg.GpnerfError, match="signed_band"):
            ev.MeshEvaluator("nowhere", 0.02, signed=True, signed_band=band)
    assert not ev.MeshEvaluator("nowhere", 0.02).signed, "off by default"


# ---- the restatement checks itself

def test_the_field_of_a_large_triangle_is_the_height_inside_its_shadow():
    """a triangle in the plane z = 0 that covers the lattice in projection: the nearest point of every lattice point is its foot, so the
    field is |z| where that is within the band and the band beyond -- to the distance function's 2^-20 (distance + diameter): the foot's
    x and y come out of float32 barycentrics of a triangle 140 across"""
    v, f = mm.f32([[-40, -40, 0], [60, -40, 0], [-40, 60, 0]]), np.array([[0, 1, 2]], np.int32)
    lo, step, dims, band = (-1.0, -1.5, -1.0), (0.25, 0.5, 0.25), (12, 10, 9), 0.6
    ref = sc.sdf_np(v, f, lo, step, dims, band)
    z = np.abs(sc.lattice_points(lo, step, dims)[..., 2])
    want = np.where(z <= np.float32(band), z, np.float32(band))
    dev = float(np.abs(ref["abs"].astype(np.float64) - want).max())
    print(f"large triangle: largest | field - |z| | {dev:.3e}, allowed {2.0 ** -20 * (0.6 + 142):.3e}")
    assert dev <= 2.0 ** -20 * (0.6 + 142) and np.array_equal(ref["face"], np.where(z <= np.float32(band), 0, -1))
    assert np.array_equal(ref["abs"][:, :, [0, 1, 2, 6, 7, 8]], want[:, :, [0, 1, 2, 6, 7, 8]]), "exact where the height dominates the sum"
    assert ref["stats"].tolist() == [1, 0, 0, 1, 12 * 10 * 5, 0, 12 * 10 * 7, 12 * 10 * 5], ref["stats"]      # k = 2 .. 6 in band; the box holds k = 1 .. 7
    assert not ref["tie"].any() and np.array_equal(ref["sdf"], ref["abs"])


def test_the_field_of_an_icosphere_is_the_spheres_within_the_chord_sag():
    """an icosphere inscribed in the sphere of radius r lies between the spheres of radius r - sag and r, sag = r - the least distance of
    a face's plane from the centre; so | field - | |P| - r | | <= sag wherever both are within the band"""
    c = sc.case("icosphere2")
    v = c["v"].astype(np.float64)
    tri = v[c["f"]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = np.abs((tri[:, 0] * n).sum(axis=1)) / np.linalg.norm(n, axis=1)
    sag = 1.0 - plane.min()
    P = sc.lattice_points(c["lo"], c["step"], c["dims"]).astype(np.float64)
    true = np.abs(np.linalg.norm(P, axis=-1) - 1.0)
    near = (true < c["band"] - sag) & (c["ref"]["face"] >= 0)
    dev = float(np.abs(c["ref"]["abs"][near] - true[near]).max())
    print(f"icosphere2: sag {sag:.5f}, largest | field - sphere | {dev:.5f} over {int(near.sum())} points")
    assert 0.005 < sag < 0.03 and near.sum() > 2500 and dev <= sag + 1e-6
    # the sign: negative exactly where the restated occupancy is set; a point inside the inner sphere is occupied
    assert np.array_equal(np.signbit(c["ref"]["sdf"]), c["occ"]) and c["occ"][np.linalg.norm(P, axis=-1) < 1.0 - sag - 0.13].all()
    assert c["ref"]["stats"][:3].tolist() == [320, 0, 0] and c["ref"]["stats"][5] == c["occ"].sum()


def test_the_cases_are_what_they_say():
    both = sc.case("both_tiers")["ref"]
    assert (both["boxes"] > sc.LARGE_POINTS).sum() == both["stats"][3] >= 12 and ((both["boxes"] > 0) & (both["boxes"] <= sc.LARGE_POINTS)).sum() > 250
    quad = sc.case("quad_large")["ref"]
    assert quad["stats"][:4].tolist() == [2, 0, 0, 2] and (quad["boxes"] >= 40 * 40 * 7).all()
    assert sc.case("beyond_band")["ref"]["stats"][:3].tolist() == [80, 0, 80]
    assert sc.case("invalid")["ref"]["stats"][:3].tolist() == [80, 4, 0]
    assert sc.case("guard")["ref"]["stats"][:3].tolist() == [80, 1, 0]
    half = sc.case("half_outside")["ref"]
    assert half["stats"][0] + half["stats"][2] == 80 and half["stats"][2] > 0 and half["stats"][4] > 150
    twice = sc.case("twice")["ref"]
    assert twice["tie"].sum() == twice["stats"][4] > 100 and set(np.unique(twice["face"]).tolist()) == {-1, 0}
    tie = sc.case("tie_box")
    P = sc.lattice_points(tie["lo"], tie["step"], tie["dims"])
    on_diagonal = (P[..., 0] == P[..., 1]) & (tie["ref"]["face"] >= 0)
    assert tie["ref"]["tie"].sum() > 100 and tie["ref"]["tie"][on_diagonal & (np.abs(P[..., 2]) < 0.5) & (np.abs(P[..., 0]) > 0.6)].all()
    plane = sc.case("plane")["ref"]
    assert (plane["abs"][:, :, [2, 6]] == 0.5).all() and (plane["face"][:, :, [2, 6]] >= 0).all(), "z = +-0.5 is exactly the band away: in"
    assert (plane["face"][:, :, [0, 1, 7, 8]] == -1).all() and (plane["abs"][:, :, [0, 1, 7, 8]] == 0.5).all(), "z = +-0.75 is beyond it"


def test_the_trilinear_restatement_equals_the_eight_corner_formula():
    rng = np.random.default_rng(11)
    dims, lo, step = (7, 6, 5), np.array([-0.3, 0.2, 1.0]), np.array([0.1, 0.25, 0.05])
    values = rng.uniform(-0.5, 0.5, dims).astype(np.float32)
    pts = mm.f32(lo + rng.uniform(0, np.array(dims) - 1, (2000, 3)) * step)
    got, want = sc.sample_np(values, lo, step, pts).astype(np.float64), sc.sample_direct(values, lo, step, pts)
    err = float(np.abs(got - want).max())
    print(f"trilinear: nested form vs the eight-corner sum, largest difference {err:.3e}")
    assert err <= 2.0 ** -24 * 0.5 + 8 * 2.0 ** -52, "one float32 rounding of a value under 0.5, and float64 noise"
    # lattice points give the stored value (a dyadic lattice: u is an integer), the last index included; outside and NaN give NaN
    lo2, step2 = np.array([-1.5, -1.5, -1.5]), np.array([0.25, 0.25, 0.25])
    ijk = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), axis=-1).reshape(-1, 3)
    at = sc.sample_np(values, lo2, step2, mm.f32(lo2 + ijk * step2))
    assert np.array_equal(at, values.reshape(-1))
    odd = mm.f32([[np.nan, 0, 0], [0, np.inf, 0], [-1.51, -1.5, -1.5], [0.01, -1.5, -1.5], [-1.5, -1.5, -0.49], [-1.5, -1.5, -0.5]])
    assert np.isnan(sc.sample_np(values, lo2, step2, odd)).tolist() == [True, True, True, True, True, False]
