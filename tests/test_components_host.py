"""CPU: the numpy restatement of the mesh components (tests/component_cases.py) against an independent second method -- a union-find
loop over the faces -- on every case, the literal numbers of the two marching-cubes cases, and the host side of the feature:
frame.parse_components, frame.read_mesh_components with every branch of the genus rule, the workspace and layout formulas and the
GPNERF_E_ARG list of gpnerf_mesh_components / _emit (the checks run before any launch, so dummy pointers do)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import component_cases as cc
import smooth_cases as sm

F = importlib.import_module("gp-nerf_amd.frame")
L = importlib.import_module("gp-nerf_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpnerf_hip.h")


def union_find_labels(faces, n_vertices):
    """the second method: a sequential union-find over the usable faces (union by smaller index, path halving)"""
    parent = list(range(n_vertices))
    referenced = [False] * n_vertices

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    for a, b, c in f[sm.usable_faces(f, n_vertices)].tolist():
        referenced[a] = referenced[b] = referenced[c] = True
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    return np.array([find(v) if referenced[v] else -1 for v in range(n_vertices)], dtype=np.int32)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_restatement_agrees_with_a_union_find_over_the_faces(name):
    v, f, ref = cc.case(name)
    label = union_find_labels(f, len(v))
    assert np.array_equal(ref["label"], label)
    roots = sorted(set(label[label >= 0].tolist()))
    assert ref["table"][:, 0].tolist() == roots and ref["stats"]["components"] == len(roots)
    number = {r: i for i, r in enumerate(roots)}
    assert ref["vertex_component"].tolist() == [number.get(int(l), -1) for l in label]
    ok = sm.usable_faces(f, len(v))
    assert ref["face_component"].tolist() == [number[int(label[a])] if u else -1 for (a, _b, _c), u in zip(f.tolist(), ok)]
    # the table's sums are the adjacency's totals
    topo = cc.adjacency(name)["stats"]
    t = ref["table"]
    assert t[:, 1].sum() == topo["vertices_referenced"] and t[:, 2].sum() == topo["edges"] and t[:, 3].sum() == topo["faces_used"]
    assert t[:, 4].sum() == topo["euler"] and t[:, 5].sum() == topo["boundary_vertices"]
    # KEEP_ALL emits the referenced vertices and the usable faces, in order
    assert ref["kept_vertices"].tolist() == np.nonzero(label >= 0)[0].tolist() and ref["kept_faces"].tolist() == np.nonzero(ok)[0].tolist()
    if len(ref["out_faces"]):
        assert np.array_equal(ref["kept_vertices"][ref["out_faces"]], f[ok])


def test_the_hand_cases_say_what_they_are_for():
    row = lambda name: cc.case(name)[2]
    assert row("bow_tie")["stats"]["components"] == 1 and row("bow_tie")["table"].tolist() == [[0, 5, 6, 2, 1, 5]]
    two = row("two_tetrahedra")
    assert two["label"].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, -1] and two["vertex_component"].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, -1]
    assert two["face_component"].tolist() == [0] * 4 + [1] * 4 and two["stats"]["largest"] == 0 and two["stats"]["closed_components"] == 2
    shuffled = row("two_tetrahedra_shuffled")
    assert shuffled["face_component"].tolist() != two["face_component"].tolist()
    for k in ("label", "vertex_component", "table"):
        assert np.array_equal(shuffled[k], two[k])
    assert shuffled["stats"] == two["stats"]
    bad = row("bad_faces")
    assert bad["label"].tolist() == [0, 0, 0, 0, 0, -1, -1] and bad["face_component"].tolist() == [0, 0, -1, -1, -1, -1, -1, 0]
    assert row("empty")["stats"]["largest"] == -1 and row("no_faces")["label"].tolist() == [-1] * 5
    for name in ("strip", "hub_last_fan"):
        assert row(name)["stats"]["components"] == 1 and (row(name)["label"] == 0).all()
    v, f = cc.mesh("hub_last_fan")
    assert (f == len(v) - 1).any(axis=1).all()                            # the hub, the highest index, is in every face
    v, f = cc.mesh("strip")
    assert np.abs(np.diff(f.astype(np.int64), axis=1)).min() > 1 and np.abs(f[1:, 0].astype(np.int64) - f[:-1, 0]).mean() > 1000


def test_the_scene_and_the_noise_surface_are_the_written_numbers():
    """derived on the CPU with this file's two methods, never from the device"""
    v, f, ref = cc.case("scene")
    assert (len(v), len(f)) == (4146, 8268)
    t = ref["table"]
    assert t[:, 0].tolist() == [0, 1, 250, 1552, 1904, 3697, 3909]
    assert t[:, 3].tolist() == [600, 600, 5472, 944, 236, 336, 80]
    assert t[:, 4].tolist() == [2, 2, 0, 2, 2, 2, 2] and t[:, 4].sum() == 12 and (t[:, 5] == 0).all()
    assert cc.stats_row(ref["stats"]) == [7, 7, 2, 5472, 2736, 0, 7, 4146, 8268]
    topo = cc.adjacency("scene")["stats"]
    assert topo["inconsistent_edges"] == 0 and topo["nonmanifold_edges"] == 0
    assert [cc.genus_np(r, 0, 0) for r in t] == [(True, 0), (True, 0), (True, 1), (True, 0), (True, 0), (True, 0), (True, 0)]      # the torus
    # the selections: the largest, and both sides of the smallest, a middle and the tied size
    for keep, n_min, comps in ((cc.KEEP_LARGEST, 1, [2]), (cc.KEEP_MIN_FACES, 80, [0, 1, 2, 3, 4, 5, 6]), (cc.KEEP_MIN_FACES, 81, [0, 1, 2, 3, 4, 5]),
                               (cc.KEEP_MIN_FACES, 336, [0, 1, 2, 3, 5]), (cc.KEEP_MIN_FACES, 337, [0, 1, 2, 3]),
                               (cc.KEEP_MIN_FACES, 600, [0, 1, 2, 3]), (cc.KEEP_MIN_FACES, 601, [2, 3]), (cc.KEEP_MIN_FACES, 6000, [])):
        sel = cc.case("scene", keep, n_min)[2]
        assert sel["stats"]["kept_components"] == len(comps) and sel["stats"]["kept_faces"] == t[comps, 3].sum() == len(sel["out_faces"])
        assert sel["stats"]["kept_vertices"] == t[comps, 1].sum() == len(sel["kept_vertices"])
        assert sorted(set(ref["vertex_component"][sel["kept_vertices"]].tolist())) == comps
    v, f, ref = cc.case("noise")
    assert (len(v), len(f)) == (50790, 108240)
    assert ref["stats"]["components"] == 263 and ref["stats"]["largest"] == 0 and ref["stats"]["largest_faces"] == 105824
    assert ref["table"][0, 0] == 0 and ref["stats"]["closed_components"] == 262
    topo = sm.read_topology(cc.adjacency("noise")["stats"])
    assert not topo["closed"] and not topo["oriented"]
    v, f, ref = cc.case("twin_blobs")
    assert ref["table"][:, 3].tolist() == [928, 928] and ref["stats"]["largest"] == 0      # a tie: the lower number
    assert cc.case("twin_blobs", cc.KEEP_LARGEST)[2]["stats"]["kept_faces"] == 928


def test_parse_components():
    for off in (None, False, 0, "0", "", " 0 ", 0.0):
        assert F.parse_components(off) is None
    assert F.parse_components("largest") == "largest" and F.parse_components(" largest ") == "largest"
    assert F.parse_components(1) == 1 and F.parse_components("44") == 44 and F.parse_components(np.int64(7)) == 7 and F.parse_components(3.0) == 3
    for bad in (True, -1, "-3", 2.5, "2.5", "smallest", "all", float("nan"), float("inf"), [1], (), {}):
        with pytest.raises(L.GpnerfError, match="knob"):
            F.parse_components(bad, "knob")


def test_read_mesh_components_and_every_branch_of_the_genus_rule():
    v, f, ref = cc.case("scene", cc.KEEP_LARGEST)
    stats, table = cc.stats_row(ref["stats"]), np.concatenate([ref["table"], np.full((3, 6), 7)])     # (rows beyond C are not read)
    topo = sm.stats_row(cc.adjacency("scene")["stats"])
    plain = F.read_mesh_components(stats)
    assert plain == ref["stats"] and list(plain) == list(L.COMPONENT_STATS) == list(cc.STATS)
    full = F.read_mesh_components(np.array(stats), table, topo)
    assert len(full["rows"]) == 7 and [r["genus"] for r in full["rows"]] == [0, 0, 1, 0, 0, 0, 0] and all(r["closed"] for r in full["rows"])
    assert full["largest_genus"] == 1 and [list(r)[:6] for r in full["rows"]] == [list(L.COMPONENT_COLS)] * 7 == [list(cc.COLS)] * 7
    assert [[r[k] for k in cc.COLS] for r in full["rows"]] == ref["table"].tolist()
    # no topology stats: closed is known, the genus is not vouched for
    assert [r["genus"] for r in F.read_mesh_components(stats, table)["rows"]] == [None] * 7
    # an inconsistent or a non-manifold edge anywhere in the mesh
    for k in ("inconsistent_edges", "nonmanifold_edges"):
        dirty = list(topo)
        dirty[sm.STATS.index(k)] = 1
        assert [r["genus"] for r in F.read_mesh_components(stats, table, dirty)["rows"]] == [None] * 7
    # an open component; an odd Euler characteristic
    opened = table.copy()
    opened[2, 5] = 4
    rows = F.read_mesh_components(stats, opened, topo)["rows"]
    assert rows[2]["closed"] is False and rows[2]["genus"] is None and rows[3]["genus"] == 0
    odd = table.copy()
    odd[3, 4] = 1
    assert F.read_mesh_components(stats, odd, topo)["rows"][3]["genus"] is None
    # no component
    none = F.read_mesh_components(cc.stats_row(cc.case("empty")[2]["stats"]), np.zeros((0, 6)), sm.stats_row(cc.adjacency("empty")["stats"]))
    assert none["rows"] == [] and none["largest_genus"] is None and none["largest"] == -1
    for bad in (dict(stats=stats[:5]), dict(stats=stats, table=table[:3]), dict(stats=stats, table=table[:, :5])):
        with pytest.raises(L.GpnerfError):
            F.read_mesh_components(**bad)
    assert "pinched" in F.read_mesh_components.__doc__.lower()


a256 = lambda b: (b + 255) // 256 * 256


@pytest.mark.parametrize("nv,nf", [(0, 0), (1, 0), (2, 5), (3, 1), (5398, 10776), (50790, 108240), (4097, 2049), (10, 300000),
                                   ((1 << 31) - 1, 715827882)])
def test_the_workspace_is_the_headers_formula(nv, nf):
    lib = L.lib()
    want = 256 + 4 * a256(4 * nv) + 2 * a256(4 * nf) + a256(48 * (nv // 3)) + a256(8 * ((max(nv, nf, 1) + 2047) // 2048))
    assert int(lib.gpnerf_mesh_components_workspace_bytes(nv, nf)) == want
    off = (C.c_int64 * 4)()
    assert lib.gpnerf_mesh_components_layout(nv, nf, off) == 0
    label, vcomp, fcomp, table = (int(o) for o in off)
    assert label == 256 and vcomp == label + a256(4 * nv) and fcomp == 256 + 4 * a256(4 * nv) and table == fcomp + 2 * a256(4 * nf)
    assert all(o % 256 == 0 for o in off) and table + 48 * (nv // 3) <= want


def test_sizes_beyond_the_limits_have_no_workspace():
    lib = L.lib()
    off = (C.c_int64 * 4)()
    for nv, nf in ((-1, 0), (0, -1), (1 << 31, 0), (4, 715827883)):
        assert int(lib.gpnerf_mesh_components_workspace_bytes(nv, nf)) == 0 and lib.gpnerf_mesh_components_layout(nv, nf, off) == -1
    assert lib.gpnerf_mesh_components_layout(4, 4, None) == -1


def test_bad_arguments_are_refused_on_the_host():
    """GPNERF_E_ARG before any launch: every call below has one thing wrong"""
    lib = L.lib()
    P = 0x1000
    nv, nf = 12, 20
    ws, adj = int(lib.gpnerf_mesh_components_workspace_bytes(nv, nf)), int(lib.gpnerf_mesh_adjacency_workspace_bytes(nv, nf))
    good = dict(faces=P, nf=nf, nv=nv, adj=P, adj_bytes=adj, keep=L.COMPONENTS_KEEP_ALL, min_faces=0, ws=P, ws_bytes=ws, stats=P)

    def count(**kw):
        a = {**good, **kw}
        return lib.gpnerf_mesh_components(a["faces"], a["nf"], a["nv"], a["adj"], a["adj_bytes"], a["keep"], a["min_faces"], a["ws"], a["ws_bytes"],
                                          a["stats"], None)

    for bad in (dict(faces=None), dict(adj=None), dict(ws=None), dict(stats=None), dict(nf=-1), dict(nv=-1), dict(nv=1 << 31), dict(nf=715827883),
                dict(keep=3), dict(keep=-1), dict(keep=L.COMPONENTS_KEEP_MIN_FACES, min_faces=0), dict(keep=L.COMPONENTS_KEEP_MIN_FACES, min_faces=-5),
                dict(ws_bytes=ws - 1), dict(adj_bytes=adj - 1), dict(ws_bytes=0)):
        assert count(**bad) == -1, bad
    e_good = dict(v=P, nv=nv, f=P, nf=nf, ws=P, ws_bytes=ws, ov=5, of=7, out_v=P, out_f=P, vmap=None, kept=None)

    def emit(**kw):
        a = {**e_good, **kw}
        return lib.gpnerf_mesh_components_emit(a["v"], a["nv"], a["f"], a["nf"], a["ws"], a["ws_bytes"], a["ov"], a["of"], a["out_v"], a["out_f"],
                                               a["vmap"], a["kept"], None)

    for bad in (dict(v=None), dict(f=None), dict(ws=None), dict(out_v=None), dict(out_f=None), dict(nv=-1), dict(nf=-1), dict(nv=1 << 31, ov=0),
                dict(ov=-1), dict(of=-1), dict(ov=nv + 1), dict(of=nf + 1), dict(ws_bytes=ws - 1)):
        assert emit(**bad) == -1, bad
    for name in ("LABEL", "VERTEX_COMPONENT", "FACE_COMPONENT", "TABLE", "KEEP_ALL", "KEEP_LARGEST", "KEEP_MIN_FACES", "HDR_STATUS", "COUNTING",
                 "COUNTED", "EMITTED", "MISMATCH", "NO_ADJACENCY"):
        assert f"#define GPNERF_COMPONENTS_{name} {getattr(L, 'COMPONENTS_' + name)}\n" in open(HEADER).read(), name
    hdr = open(HEADER).read()
    for i, n in enumerate(L.COMPONENT_STATS):
        assert f"#define GPNERF_COMPONENTS_{n.upper()} {i}\n" in hdr, n
    for i, n in enumerate(L.COMPONENT_COLS):
        assert f"#define GPNERF_COMPONENT_{n.upper()} {i}\n" in hdr, n
    assert f"#define GPNERF_COMPONENT_STATS {len(L.COMPONENT_STATS)}\n" in hdr and f"#define GPNERF_COMPONENT_COLS {len(L.COMPONENT_COLS)}\n" in hdr


def test_the_out_of_scope_sentences_are_gone():
    hdr = open(HEADER).read()
    assert "a label propagation over a mesh needs" not in hdr and "genus are not counted" not in hdr
    assert "not counted" not in F.read_mesh_topology.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Out of scope: connected components and the genus" not in design and "4.15" in design
