"""CPU: the numpy restatement of the mesh repair (tests/repair_cases.py) on every case -- the two count identities, the maps inverse to
each other, idempotence, and what each hand case is there for --, and the host side of the feature: frame.read_mesh_repair, the
workspace formula against its stated terms and the GPNERF_E_ARG list of gpnerf_mesh_repair / _emit (the checks run before any
launch, so dummy pointers do)."""
import importlib
import os

import numpy as np
import pytest

import repair_cases as rc
import smooth_cases as sm

F = importlib.import_module("gp-nerf_amd.frame")
L = importlib.import_module("gp-nerf_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpnerf_hip.h")


@pytest.mark.parametrize("name", list(rc.CASES))
def test_the_restatements_own_properties(name):
    v, f, kw, ref = rc.case(name)
    s = ref["stats"]
    assert len(f) == s["faces_out"] + s["faces_invalid"] + s["faces_unkeyable"] + s["faces_collapsed"] + s["faces_duplicate"]
    assert len(v) == s["vertices_out"] + s["vertices_welded"] + s["vertices_unkeyable"] + s["vertices_unreferenced"]
    assert all(x >= 0 for x in s.values())
    kept, vmap, fmap = ref["kept_vertices"], ref["vertex_map"], ref["face_map"]
    assert len(kept) == s["vertices_out"] == len(ref["vertices"]) and len(fmap) == s["faces_out"] == len(ref["faces"]) == len(ref["face_patch"])
    # the maps are inverse to each other; a welded vertex maps to where its representative went
    assert np.array_equal(vmap[kept], np.arange(len(kept))) and (np.diff(kept) > 0).all() and (np.diff(fmap) > 0).all()
    keyable = ref["rep"] >= 0
    assert np.array_equal(vmap[keyable], vmap[ref["rep"][keyable]]) and (vmap[~keyable] == -1).all()
    assert ref["vertices"].tobytes() == v[kept].tobytes()
    live = ref["face_fate"] <= rc.KEPT_FLIPPED
    assert np.array_equal(np.nonzero(live)[0], fmap) and int((ref["face_fate"] == rc.KEPT_FLIPPED).sum()) == s["faces_flipped"]
    # an output face is the original's corners through vertex_map, (a, c, b) when flipped
    through = vmap[f[fmap].astype(np.int64)].reshape(-1, 3)
    swap = ref["face_fate"][fmap] == rc.KEPT_FLIPPED
    through[swap] = through[swap][:, [0, 2, 1]]
    assert np.array_equal(through, ref["faces"]) and (ref["faces"] >= 0).all()
    assert (ref["face_patch"] <= fmap).all() and set(ref["face_patch"].tolist()) <= set(fmap.tolist())
    if kw["orient"]:
        assert s["patches"] == len(set(ref["face_patch"].tolist())) and s["patches_closed"] <= s["patches"]
    # idempotence: repairing the repaired mesh changes nothing
    again = rc.repair_np(ref["vertices"], ref["faces"], **kw)
    assert not rc.changed(again["stats"]), again["stats"]
    assert again["vertices"].tobytes() == ref["vertices"].tobytes() and np.array_equal(again["faces"], ref["faces"])
    for k in ("patches", "patches_closed", "patches_unorientable", "patches_undecided", "edges_nonmanifold"):
        assert again["stats"][k] == s[k], k
    assert again["stats"]["patches_inverted"] == 0


def test_the_hand_cases_say_what_they_are_for():
    ref = lambda name: rc.case(name)[3]
    s = ref("cube_soup")["stats"]
    assert (s["vertices_out"], s["faces_out"], s["vertices_welded"], s["patches"], s["patches_closed"], s["faces_flipped"]) == (8, 12, 28, 1, 1, 0)
    v, f = rc.case("cube_soup")[:2]
    before, after = sm.adjacency_np(f, len(v))["stats"], sm.read_topology(sm.adjacency_np(ref("cube_soup")["faces"], 8)["stats"])
    assert before["boundary_edges"] == 36 and after["watertight"] and after["euler"] == 2
    s = ref("signed_zero")["stats"]
    assert (s["vertices_out"], s["vertices_welded"], s["patches_closed"]) == (4, 8, 1)
    nan = ref("nan_vertex")
    assert nan["stats"]["vertices_unkeyable"] == 1 and nan["stats"]["faces_unkeyable"] == 3 and nan["vertex_map"][5] == -1
    assert np.array_equal(nan["faces"][:4], sm.tetrahedron()[1]) and nan["stats"]["patches"] == 2 and nan["stats"]["patches_closed"] == 1
    g = ref("grid")
    assert g["rep"].tolist() == [0, 1, 2, 2, 4, 5, -1, 7, 7]
    assert np.where(g["face_fate"] == rc.KEPT_FLIPPED, rc.KEPT, g["face_fate"]).tolist() == [rc.KEPT, rc.COLLAPSED, rc.KEPT, rc.DUPLICATE, rc.UNKEYABLE, rc.COLLAPSED, rc.KEPT, rc.KEPT]
    v, f, group = rc.crowd()
    c = ref("crowd")
    lowest = np.array([np.nonzero(group == k)[0].min() for k in range(64)])
    assert np.array_equal(c["rep"], lowest[group]) and np.array_equal(c["kept_vertices"], np.sort(lowest)) and c["stats"]["vertices_welded"] == 4032
    assert c["stats"]["faces_duplicate"] == 192
    s = ref("strip")["stats"]
    assert s["vertices_out"] == 4502 > 2 * 2048 and s["faces_out"] == 4500 and s["faces_flipped"] == 1500 and s["patches"] == 1
    b = ref("bad_faces")
    assert b["face_fate"].tolist() == [0, 0, rc.INVALID, rc.INVALID, rc.INVALID, rc.COLLAPSED, rc.COLLAPSED, 0, rc.DUPLICATE, rc.DUPLICATE]
    assert b["stats"]["vertices_unreferenced"] == 2 and b["vertex_map"].tolist() == [0, 1, 2, 3, 4, -1, -1]
    sphere = ref("flipped_sphere")
    cv, cf = rc.ico(2)
    assert rc.det_sum(cv, cf) > 0, "the icosphere is wound outward"
    assert sphere["stats"]["faces_flipped"] == 160 and sphere["vertices"][sphere["faces"]].tobytes() == cv[cf].tobytes()
    assert sm.adjacency_np(sphere["faces"], len(cv))["stats"]["inconsistent_edges"] == 0
    s = ref("inside_out")["stats"]
    assert s["patches_inverted"] == 1 and s["faces_flipped"] == 80 == s["faces_out"]
    s = ref("inside_out_not_outward")["stats"]
    assert s["patches_inverted"] == 0 and s["faces_flipped"] == 0 and not rc.changed(s)
    m = ref("moebius")
    assert m["stats"]["patches_unorientable"] == 1 and m["stats"]["patches"] == 1 and m["stats"]["faces_flipped"] == 0
    assert np.array_equal(m["faces"], rc.moebius()[1])
    clean = rc.sheet()[1]
    third = ref("open_sheet_third")
    assert third["stats"]["faces_flipped"] == 96 and np.array_equal(third["faces"], clean)
    half = ref("open_sheet_half")
    assert half["stats"]["faces_flipped"] == 144 and np.array_equal(half["faces"], clean)                 # the root, face 0, was not flipped: its side stays
    half = ref("open_sheet_half_root_flipped")
    assert half["stats"]["faces_flipped"] == 144 and np.array_equal(half["faces"], clean[:, [0, 2, 1]])    # the root was: the others follow it
    s = ref("shared_edge")["stats"]
    assert (s["edges_nonmanifold"], s["patches"], s["patches_closed"], s["faces_flipped"], s["patches_inverted"]) == (1, 2, 2, 0, 0)
    n = ref("nested")
    assert n["stats"]["patches"] == 2 and n["stats"]["patches_inverted"] == 1 and n["stats"]["faces_flipped"] == 80
    assert (n["face_fate"][:80] == rc.KEPT).all() and (n["face_fate"][80:] == rc.KEPT_FLIPPED).all()
    s = ref("flat_closed")["stats"]
    assert (s["faces_out"], s["patches"], s["patches_closed"], s["patches_undecided"], s["faces_flipped"]) == (2, 1, 1, 1, 0)
    assert ref("empty")["stats"] == dict.fromkeys(rc.STATS, 0)
    s = ref("no_faces")["stats"]
    assert s["vertices_unreferenced"] == 5 and sum(s.values()) == 5
    soup = ref("mc_sphere_soup")
    cv, cf = rc.mc_sphere_clean()
    top = sm.read_topology(sm.adjacency_np(soup["faces"], len(soup["vertices"]))["stats"])
    assert top["watertight"] and top["euler"] == 2 and len(soup["vertices"]) == len(cv) and soup["stats"]["patches_closed"] == 1
    assert rc.det_sum(soup["vertices"], soup["faces"]) > 0


def test_read_mesh_repair():
    for name in ("cube_soup", "inside_out_not_outward", "bad_faces", "empty"):
        ref = rc.case(name)[3]["stats"]
        got = F.read_mesh_repair(np.array(rc.stats_row(ref)))
        assert got.pop("changed") == rc.changed(ref) and got == ref and list(got) == list(L.REPAIR_STATS) == list(rc.STATS)
    assert F.read_mesh_repair([0] * 9 + [1] + [0] * 6)["changed"] and not F.read_mesh_repair([5, 5] + [0] * 8 + [1] * 6)["changed"]
    with pytest.raises(L.GpnerfError):
        F.read_mesh_repair([0] * 15)
    assert L.REPAIR_FATES.index("kept_flipped") == rc.KEPT_FLIPPED and L.REPAIR_FATES.index("duplicate") == rc.DUPLICATE


a256 = lambda b: (b + 255) // 256 * 256


def capacity(n):
    c = 64
    while c < 2 * n:
        c *= 2
    return c


@pytest.mark.parametrize("nv,nf", [(0, 0), (1, 0), (0, 3), (36, 12), (31, 32), (32, 33), (983040, 327680), (4097, 2049), (10, 300000),
                                   (1 << 30, 715827882)])
def test_the_workspace_is_the_headers_formula(nv, nf):
    cv, cf, ce = capacity(nv), capacity(nf), capacity(3 * nf)
    want = (256 + 2 * a256(4 * nv) + a256(4 * cv) + 2 * a256(nf) + 3 * a256(4 * nf) + a256(4 * cf) + 2 * a256(8 * ce) + 3 * a256(4 * ce) +
            a256(56 * nf) + a256(8 * ((max(nv, nf, 1) + 2047) // 2048)))
    assert int(L.lib().gpnerf_mesh_repair_workspace_bytes(nv, nf)) == want
    assert cv >= 64 and cv >= 2 * nv and (cv == 64 or cv < 4 * nv) and cv & (cv - 1) == 0


def test_sizes_beyond_the_limits_have_no_workspace():
    lib = L.lib()
    for nv, nf in ((-1, 0), (0, -1), ((1 << 30) + 1, 0), (4, 715827883)):
        assert int(lib.gpnerf_mesh_repair_workspace_bytes(nv, nf)) == 0


def test_bad_arguments_are_refused_on_the_host():
    """GPNERF_E_ARG before any launch: every call below has one thing wrong"""
    lib = L.lib()
    P = 0x1000
    nv, nf = 12, 20
    ws = int(lib.gpnerf_mesh_repair_workspace_bytes(nv, nf))
    every = L.REPAIR_WELD | L.REPAIR_DROP_DUPLICATES | L.REPAIR_ORIENT | L.REPAIR_OUTWARD
    good = dict(v=P, nv=nv, f=P, nf=nf, tol=0.0, flags=every, ws=P, ws_bytes=ws, stats=P)

    def count(**kw):
        a = {**good, **kw}
        return lib.gpnerf_mesh_repair(a["v"], a["nv"], a["f"], a["nf"], a["tol"], a["flags"], a["ws"], a["ws_bytes"], a["stats"], None)

    for bad in (dict(v=None), dict(f=None), dict(ws=None), dict(stats=None), dict(nv=-1), dict(nf=-1), dict(nv=(1 << 30) + 1), dict(nf=715827883),
                dict(ws_bytes=ws - 1), dict(ws_bytes=0), dict(flags=16), dict(flags=every | 1 << 31), dict(flags=L.REPAIR_OUTWARD),
                dict(flags=L.REPAIR_OUTWARD | L.REPAIR_WELD), dict(tol=-1e-9), dict(tol=float("inf")), dict(tol=float("nan"))):
        assert count(**bad) == -1, bad
    e_good = dict(v=P, nv=nv, f=P, nf=nf, ws=P, ws_bytes=ws, out_v=P, ov=5, out_f=P, of=7)

    def emit(**kw):
        a = {**e_good, **kw}
        return lib.gpnerf_mesh_repair_emit(a["v"], a["nv"], a["f"], a["nf"], a["ws"], a["ws_bytes"], a["out_v"], a["ov"], a["out_f"], a["of"],
                                           None, None, None, None, None, None)

    for bad in (dict(v=None), dict(f=None), dict(ws=None), dict(out_v=None), dict(out_f=None), dict(nv=-1), dict(nf=-1), dict(nv=(1 << 30) + 1, ov=0),
                dict(ov=-1), dict(of=-1), dict(ov=nv + 1), dict(of=nf + 1), dict(ws_bytes=ws - 1)):
        assert emit(**bad) == -1, bad
    hdr = open(HEADER).read()
    for i, n in enumerate(L.REPAIR_STATS):
        assert f"#define GPNERF_REPAIR_{n.upper()} {i}\n" in hdr, n
    for i, n in enumerate(L.REPAIR_FATES):
        assert f"#define GPNERF_REPAIR_{n.upper()} {i}\n" in hdr, n
    assert f"#define GPNERF_REPAIR_STATS {len(L.REPAIR_STATS)}\n" in hdr
    for name in ("WELD", "DROP_DUPLICATES", "ORIENT", "OUTWARD"):
        assert f"#define GPNERF_REPAIR_{name} {getattr(L, 'REPAIR_' + name)}u\n" in hdr, name
    for name in ("HDR_STATUS", "COUNTING", "COUNTED", "EMITTED", "MISMATCH", "NO_COUNT"):
        assert f"#define GPNERF_REPAIR_{name} {getattr(L, 'REPAIR_' + name)}\n" in hdr, name


def test_the_wrappers_check_their_keywords_before_the_device():
    with pytest.raises(L.GpnerfError, match="outward needs orient"):
        F._repair_flags(True, True, False, True)
    assert F._repair_flags(True, True, True, True) == 15 and F._repair_flags(False, False, False, False) == 0
    ev = importlib.import_module("gp-nerf_amd.evaluator")
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(L.GpnerfError, match="repair_tol"):
            ev.MeshEvaluator("unused", 0.02, repair_gt=True, repair_tol=bad)
    assert "DROPPED" in F.repair_mesh_object.__doc__ and "4.22" in open(os.path.join(ROOT, "DESIGN.md")).read()
