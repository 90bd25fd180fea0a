"""CPU: the voxeliser's entry points refuse bad arguments on the host before anything is launched, the workspace formula, the wrappers
refuse CPU tensors, and self-checks of the numpy restatement (tests/voxelize_cases.py) the GPU tests compare against."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import mesh_metric_cases as mm
import voxelize_cases as vc

P = 0x1000                                                   # a non-null dummy: argument checks never dereference
PARITY, NONZERO = 0, 1


def _dims(*d):
    return (C.c_int32 * 3)(*d)


def _lat(L, lo=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0)):
    return np.array(list(lo) + list(step), np.float64).ctypes.data_as(L.DP), np.array(list(lo) + list(step), np.float64)


def test_voxelize_rejects_bad_arguments_on_the_host(pkg):
    L = pkg._lib
    lib = L.lib()
    good_lat = np.array([0, 0, 0, 1, 1, 1], np.float64)
    big = 1 << 40

    def call(vertices=P, nv=10, faces=P, nf=5, lat=good_lat, dims=(12, 10, 9), rule=PARITY, ws=P, ws_bytes=big, bits=P, stats=P):
        lp = None if lat is None else np.ascontiguousarray(lat, np.float64).ctypes.data_as(L.DP)
        return lib.gpnerf_mesh_voxelize(vertices, nv, faces, nf, lp, None if dims is None else _dims(*dims), rule, ws, ws_bytes, bits, stats, None)

    lat = lambda i, v: np.concatenate([good_lat[:i], [v], good_lat[i + 1:]])
    for bad in (dict(vertices=None), dict(faces=None), dict(lat=None), dict(dims=None), dict(ws=None), dict(bits=None), dict(stats=None),
                dict(nv=-1), dict(nf=-1), dict(nf=1 << 31), dict(nv=1 << 31), dict(rule=2), dict(rule=-1),
                dict(dims=(0, 10, 9)), dict(dims=(12, -1, 9)), dict(dims=(12, 10, 0)), dict(dims=(1 << 10, 1 << 10, (1 << 8) + 1)),
                dict(dims=(1 << 20, 1 << 20, 1)), dict(lat=lat(0, np.nan)), dict(lat=lat(2, np.inf)), dict(lat=lat(3, 0.0)),
                dict(lat=lat(4, -1.0)), dict(lat=lat(5, np.nan)), dict(lat=lat(5, np.inf))):
        assert call(**bad) == -1, bad
    for rule in (PARITY, NONZERO):
        need = int(lib.gpnerf_mesh_voxelize_workspace_bytes(5, _dims(12, 10, 9), rule))
        assert need > 0 and call(rule=rule, ws_bytes=need - 1) == -1 and call(rule=rule, ws_bytes=0) == -1


def test_the_packed_cube_entry_points_reject_bad_arguments_on_the_host(pkg):
    L = pkg._lib
    lib = L.lib()
    d, bad_d = _dims(12, 10, 9), _dims(12, 0, 9)
    lp, _ = _lat(L)
    assert lib.gpnerf_voxel_from_cube(None, d, 0.02, P, None) == -1 and lib.gpnerf_voxel_from_cube(P, d, 0.02, None, None) == -1
    assert lib.gpnerf_voxel_from_cube(P, None, 0.02, P, None) == -1 and lib.gpnerf_voxel_from_cube(P, bad_d, 0.02, P, None) == -1
    assert lib.gpnerf_voxel_unpack(None, d, P, None) == -1 and lib.gpnerf_voxel_unpack(P, d, None, None) == -1
    assert lib.gpnerf_voxel_unpack(P, None, P, None) == -1 and lib.gpnerf_voxel_unpack(P, bad_d, P, None) == -1
    assert lib.gpnerf_voxel_stats(None, P, d, P, None) == -1 and lib.gpnerf_voxel_stats(P, P, d, None, None) == -1
    assert lib.gpnerf_voxel_stats(P, None, None, P, None) == -1 and lib.gpnerf_voxel_stats(P, None, bad_d, P, None) == -1

    def contains(bits=P, dims=d, lat=lp, points=P, n=7, out=P):
        return lib.gpnerf_voxel_contains(bits, dims, lat, points, n, out, None)

    bad_step = np.array([0, 0, 0, 1, 0, 1], np.float64).ctypes.data_as(L.DP)
    for bad in (dict(bits=None), dict(dims=None), dict(dims=bad_d), dict(lat=None), dict(lat=bad_step), dict(points=None), dict(out=None),
                dict(n=-1), dict(n=1 << 31)):
        assert contains(**bad) == -1, bad
    assert contains(points=None, out=None, n=0) == 0, "no points: nothing to launch"


def test_the_workspace_formula(pkg):
    """include/gpnerf_hip.h: 256 + align256(4 nx ny T) + align256(4 n_faces), T = nz // 32 + 1 toggle words per column under PARITY and
    nz + 1 counts under NONZERO: the header, the toggle rows (nz + 1 places each), a list entry per face at worst; host arithmetic only;
    0 for what the call refuses"""
    lib = pkg._lib.lib()
    ws = lambda nf, d, rule: int(lib.gpnerf_mesh_voxelize_workspace_bytes(nf, _dims(*d), rule))
    al = lambda b: (b + 255) // 256 * 256
    for nf, d in ((0, (1, 1, 1)), (12, (12, 10, 9)), (12, (12, 10, 31)), (12, (12, 10, 32)), (12, (12, 10, 33)), (12, (12, 10, 64)),
                  (108240, (34, 34, 34)), (327680, (140, 90, 400)), (2 ** 31 - 1, (1 << 10, 1 << 10, 1 << 8)), (7, (1, 1, 1 << 28))):
        assert ws(nf, d, PARITY) == 256 + al(4 * d[0] * d[1] * (d[2] // 32 + 1)) + al(4 * nf), (nf, d)
        assert ws(nf, d, NONZERO) == 256 + al(4 * d[0] * d[1] * (d[2] + 1)) + al(4 * nf), (nf, d)
    for refused in ((-1, (4, 4, 4), 0), (1 << 31, (4, 4, 4), 0), (5, (0, 4, 4), 0), (5, (4, 4, -2), 1), (5, (4, 4, 4), 2),
                    (5, (1 << 10, 1 << 10, (1 << 8) + 1), 0), (5, (1 << 16, 1 << 16, 1), 1)):
        assert ws(*refused) == 0, refused
    assert int(lib.gpnerf_mesh_voxelize_workspace_bytes(5, None, 0)) == 0


def test_the_header_and_the_binding_name_the_same_constants(pkg):
    import os
    import re
    L = pkg._lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpnerf_hip.h")).read()
    value = lambda name: int(re.search(rf"#define GPNERF_VOXEL_{name} (\d+)\b", hdr).group(1))
    assert [value(n.upper()) for n in L.VOXEL_STATS] == list(range(6)) and value("STATS") == len(L.VOXEL_STATS) == len(vc.STATS)
    assert tuple(L.VOXEL_STATS) == vc.STATS
    assert (value("PARITY"), value("NONZERO")) == (L.VOXEL_PARITY, L.VOXEL_NONZERO) == (L.VOXEL_RULES["parity"], L.VOXEL_RULES["nonzero"])
    assert (value("A"), value("B"), value("BOTH"), value("EITHER"), value("COUNTS")) == (L.VOXEL_A, L.VOXEL_B, L.VOXEL_BOTH, L.VOXEL_EITHER,
                                                                                        L.VOXEL_COUNTS)


def test_cpu_tensors_are_refused(pkg):
    F = importlib.import_module("gp-nerf_amd.frame")
    v, f = vc.box_mesh(*vc.BOX)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.voxelize_mesh(torch.from_numpy(v), torch.from_numpy(f), (0, 0, 0), (1, 1, 1), (12, 10, 9))
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.voxelize_cube(torch.zeros((4, 4, 4)))
    grid = F.VoxelGrid(torch.zeros((4, 4, 1), dtype=torch.int32), (4, 4, 4))
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        F.voxel_stats(grid)
    with pytest.raises(pkg.GpnerfError, match="no CPU fallback"):
        grid.contains(torch.zeros((3, 3)))
    with pytest.raises(pkg.GpnerfError, match="rule"):
        F.voxelize_mesh(torch.from_numpy(v), torch.from_numpy(f), (0, 0, 0), (1, 1, 1), (12, 10, 9), rule="even-odd")
    with pytest.raises(pkg.GpnerfError, match="dims"):
        F.VoxelGrid(None, (4, 0, 4))
    with pytest.raises(pkg.GpnerfError, match="step"):
        F.VoxelGrid(None, (4, 4, 4), step=(1, 0, 1))
    ev = importlib.import_module("gp-nerf_amd.evaluator")
    with pytest.raises(pkg.GpnerfError, match="volume_rule"):
        ev.MeshEvaluator("nowhere", 0.02, volume=True, volume_rule="odd")


def test_read_volume_metrics_on_hand_made_counts():
    F = importlib.import_module("gp-nerf_amd.frame")
    r = F.read_volume_metrics(np.array([40, 50, 30, 60]), (0.5, 0.25, 2.0))
    assert r == {"volume_a": 10.0, "volume_b": 12.5, "iou": 0.5, "precision": 0.75, "recall": 0.6}
    assert F.read_volume_metrics(torch.tensor([0, 0, 0, 0]), (1, 1, 1)) == {"volume_a": 0.0, "volume_b": 0.0, "iou": 1.0, "precision": 1.0,
                                                                           "recall": 1.0}
    assert F.read_volume_metrics([8, 0, 0, 8], (1, 1, 1))["iou"] == 0.0


# ---- the restatement checks itself

@pytest.mark.parametrize("rule", ["parity", "nonzero"])
@pytest.mark.parametrize("name", vc.FIELDS)
def test_the_round_trip_through_marching_cubes_is_exact(name, rule):
    """voxelising the marching-cubes mesh of a cube on that cube's own lattice gives back cube > iso, point for point: every crossing
    of a column is a vertex on a z edge of the lattice, owned by exactly one face of its fan, with that vertex's float32 z"""
    f = vc.field(name)
    v, faces = vc.field_mesh(name)
    ref = vc.voxelize_np(v, faces, (0, 0, 0), (1, 1, 1), f.shape, rule)
    inside = f > vc.ISO
    print(f"{name} {rule}: {len(faces)} faces, stats {ref['stats'].tolist()}, points that differ {int((ref['occ'] != inside).sum())}")
    assert np.array_equal(ref["occ"], inside) and ref["stats"][5] == inside.sum() and ref["stats"][4] == 0
    assert np.array_equal(vc.unpack_bits(ref["bits"], f.shape[2]), inside)
    # every column's crossings are its inside / outside changes along z (the border is outside)
    assert ref["stats"][3] == (np.diff(np.pad(inside, ((0, 0), (0, 0), (1, 1))).astype(np.int8), axis=2) != 0).sum()
    if name == "all_cases":
        assert len(faces) > 100000 and f.shape == (34, 34, 34)


def test_a_box_on_lattice_planes_fills_half_open():
    for rule in ("parity", "nonzero"):
        ref = vc.case("box_nz9", rule)["ref"]
        want = np.zeros((12, 10, 9), bool)
        want[2:7, 3:6, 2:6] = True                            # the minimum side is in, the maximum side is out
        assert ref["stats"].tolist() == [4, 0, 8, 30, 0, 60] and np.array_equal(ref["occ"], want)


def test_two_overlapping_boxes_cancel_under_parity_and_unite_under_nonzero():
    a = np.zeros((12, 12, 9), bool)
    b = np.zeros((12, 12, 9), bool)
    a[2:7, 3:6, 2:6] = True
    b[4:9, 4:9, 4:8] = True
    par, non = vc.case("two_boxes", "parity")["ref"], vc.case("two_boxes", "nonzero")["ref"]
    assert par["stats"][5] == 136 and np.array_equal(par["occ"], a ^ b)
    assert non["stats"][5] == 148 and np.array_equal(non["occ"], a | b)
    assert par["stats"][4] == 0 and non["stats"][4] == 0
    twice_p, twice_n = vc.case("twice", "parity")["ref"], vc.case("twice", "nonzero")["ref"]
    assert twice_p["stats"][5] == 0 and np.array_equal(twice_n["occ"], vc.case("box_nz9", "nonzero")["ref"]["occ"])


def test_parity_does_not_depend_on_the_order_or_the_orientation_of_the_faces():
    c = vc.case("both_tiers", "parity")
    rng = np.random.default_rng(4)
    f = c["f"][rng.permutation(len(c["f"]))].copy()
    flip = rng.random(len(f)) < 0.5
    f[flip] = f[flip][:, ::-1]
    again = vc.voxelize_np(c["v"], f, c["lo"], c["step"], c["dims"], "parity")
    assert flip.sum() > 100 and np.array_equal(again["bits"], c["ref"]["bits"]) and np.array_equal(again["stats"], c["ref"]["stats"])
    # NONZERO does not depend on the order either (it does on a flip of SOME faces, which it is for)
    n = vc.case("both_tiers", "nonzero")
    perm = vc.voxelize_np(n["v"], n["f"][rng.permutation(len(n["f"]))], n["lo"], n["step"], n["dims"], "nonzero")
    assert np.array_equal(perm["bits"], n["ref"]["bits"])


def test_the_occupied_volume_is_the_meshs_volume_within_the_surface_layer():
    """|OCCUPIED x the product of the steps - the divergence theorem's volume| <= area x |step|: a lattice point's cell (the box of one
    step around it) is counted wrongly only when the surface passes through it, and those cells lie within half a cell diagonal of
    the surface on either side: a layer of volume area x |step| at most"""
    for rule in ("parity", "nonzero"):
        c = vc.case("anisotropic", rule)
        got = float(c["ref"]["stats"][5]) * float(np.prod(c["step"]))
        true = vc.mesh_volume(c["v"], c["f"])
        bound = vc.mesh_area(c["v"], c["f"]) * float(np.linalg.norm(c["step"]))
        print(f"anisotropic {rule}: lattice volume {got:.6f}, mesh volume {true:.6f}, difference {abs(got - true):.6f}, bound {bound:.6f}")
        assert 0.1 < true < 0.13 and abs(got - true) <= bound and c["ref"]["stats"][4] == 0


def test_open_meshes_and_faces_outside_the_lattice():
    for rule in ("parity", "nonzero"):
        h = vc.case("hemisphere", rule)["ref"]
        assert h["stats"][4] > 0 and h["stats"][4] == h["open"].sum()
        z = vc.case("zero_faces", rule)["ref"]
        assert not z["stats"].any() and not z["bits"].any()
        d = vc.case("degenerate", rule)["ref"]
        assert d["stats"][:3].tolist() == [4, 5, 10] and np.array_equal(d["occ"], vc.case("box_nz9", rule)["ref"]["occ"])
        o = vc.case("outside_xy", rule)["ref"]
        assert o["stats"][0] == 16 and o["stats"][5] == 60 + 2 * 2 * 4          # the cut box keeps its columns 10..11 x 8..9
        a = vc.case("above_below", rule)["ref"]
        assert a["occ"][2:7, 3:6, :].all(), "a box through the whole lattice fills its columns"
        assert a["stats"][4] >= 2, "the lone face above makes its columns open (and fills them), the one below only open"
    assert vc.case("box_large", "parity")["ref"]["stats"].tolist() == [4, 0, 8, 1800, 0, 30 * 30 * 14]
    for rule in ("parity", "nonzero"):
        assert vc.case("wide_large", rule)["ref"]["stats"].tolist() == [4, 0, 8, 2 * 40 * 9, 0, 40 * 9 * 14]
        w = vc.case("wedge_large", rule)
        assert w["ref"]["stats"].tolist() == [4, 0, 0, 610, 0, 1315] and not w["ref"]["open"].any() and 1e-4 < w["ref"]["margin"] < 2e-4
        turned = vc.voxelize_np(w["v"], w["f"][:, ::-1], w["lo"], w["step"], w["dims"], rule)
        assert np.array_equal(turned["occ"], w["ref"]["occ"]), "occupancy does not change when every face is reversed"
    t = vc.case("tall", "parity")
    assert t["dims"][2] // 32 + 1 > 64


def test_contains_and_counts_restated():
    occ = vc.case("box_nz9", "parity")["ref"]["occ"]
    pts = mm.f32([[2.0, 3.0, 2.0], [6.49, 5.49, 5.49], [6.51, 5.0, 5.0], [1.5, 3.0, 2.0], [2.5, 3.0, 2.0], [-1.0, 3.0, 2.0], [np.nan, 3.0, 2.0],
                  [4.0, 4.0, 100.0], [4.0, np.inf, 3.0]])
    assert vc.contains_np(occ, (0, 0, 0), (1, 1, 1), pts).tolist() == [1, 1, 0, 1, 1, 0, 0, 0, 0]      # 1.5 and 2.5 both round to 2 (half to even)
    other = np.roll(occ, 1, axis=0)
    assert vc.voxel_counts_np(occ, other).tolist() == [60, 60, 48, 72] and vc.voxel_counts_np(occ).tolist() == [60, 0, 0, 60]
