"""A numpy restatement of the mesh repair of csrc/gpnerf_meshrepair.hip (THE DEFINITION in include/gpnerf_hip.h, step by step: dicts
for the key groups, the face fates in a loop over the faces, a sweep to a fixed point for the patches and their parities, Python
integers for the volume) and the meshes the tests run it on."""
import functools

import numpy as np

import mesh_metric_cases as mm
import simplify_cases as sc
import smooth_cases as sm

STATS = ("vertices_out", "faces_out", "vertices_welded", "vertices_unkeyable", "vertices_unreferenced", "faces_invalid", "faces_unkeyable",
         "faces_collapsed", "faces_duplicate", "faces_flipped", "edges_nonmanifold", "patches", "patches_closed", "patches_unorientable",
         "patches_inverted", "patches_undecided")
KEPT, KEPT_FLIPPED, INVALID, UNKEYABLE, COLLAPSED, DUPLICATE = range(6)
CHANGES = ("vertices_welded", "vertices_unkeyable", "vertices_unreferenced", "faces_invalid", "faces_unkeyable", "faces_collapsed",
           "faces_duplicate", "faces_flipped")


def key_np(p, tol):
    """step 1: the key of one float32 vertex, None for an unkeyable one"""
    if not np.isfinite(p).all():
        return None
    if tol > 0:
        d = p.astype(np.float64) / np.float64(tol)
        if not (np.abs(d) < 2.0 ** 62).all():
            return None
        return tuple(int(x) for x in np.floor(d))
    bits = p.view(np.uint32)
    return tuple(0 if int(b) == 0x80000000 else int(b) for b in bits)


def quantise_np(points, lo, hi):
    """step 6's grid: int64 [n, 3] of float32 points, from the float32 box (lo, hi) [3]"""
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    c = (lo + hi) / np.float64(2.0)
    ext = np.max(hi - lo)
    if not ext > 0:
        return np.zeros(points.shape, dtype=np.int64)
    scale = np.float64(1048574.0) / ext
    return np.rint((points.astype(np.float64) - c) * scale).astype(np.int64)


def det_int(a, b, c):
    a, b, c = ([int(x) for x in p] for p in (a, b, c))
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))


def repair_np(vertices, faces, tol=0.0, weld=True, drop_duplicates=True, orient=True, outward=True):
    """steps 1 - 7: {"vertices" float32 [n', 3], "faces" int32 [m', 3], "stats" dict, "vertex_map", "kept_vertices", "face_map",
    "face_patch" int32, "face_fate" uint8, "rep" int32}"""
    assert orient or not outward
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv, nf = len(v), len(f)
    # 1, 2: keys and representatives
    keys = [key_np(v[i], tol) for i in range(nv)]
    first = {}
    rep = np.full(nv, -1, dtype=np.int64)
    for i, k in enumerate(keys):
        if k is not None:
            rep[i] = first.setdefault(k, i) if weld else i
    # 3: the fates
    fate = np.zeros(nf, dtype=np.uint8)
    seen = set()
    for i, (a, b, c) in enumerate(f.tolist()):
        if not all(0 <= x < nv for x in (a, b, c)):
            fate[i] = INVALID
        elif min(rep[a], rep[b], rep[c]) < 0:
            fate[i] = UNKEYABLE
        elif len({rep[a], rep[b], rep[c]}) < 3:
            fate[i] = COLLAPSED
        elif drop_duplicates and frozenset((rep[a], rep[b], rep[c])) in seen:
            fate[i] = DUPLICATE
        else:
            seen.add(frozenset((rep[a], rep[b], rep[c])))
    live = np.nonzero(fate == KEPT)[0]
    corners = {int(i): [int(rep[x]) for x in f[i]] for i in live}
    # 4: the output vertices
    kept_vertices = np.array(sorted({x for c in corners.values() for x in c}), dtype=np.int64)
    new = np.full(nv, -1, dtype=np.int64)
    new[kept_vertices] = np.arange(len(kept_vertices))
    vertex_map = np.where(rep >= 0, new[np.maximum(rep, 0)], -1)
    # 5: edges, patches, parities
    stats = dict.fromkeys(STATS, 0)
    flip = {i: 0 for i in corners}
    patch = {i: i for i in corners}
    if orient:
        edges = {}
        for i, c in corners.items():
            for k in range(3):
                a, b = c[k], c[(k + 1) % 3]
                edges.setdefault((min(a, b), max(a, b)), []).append((i, 1 if a < b else 0))
        stats["edges_nonmanifold"] = sum(len(h) >= 3 for h in edges.values())
        joined = [(h[0][0], h[1][0], 1 if h[0][1] == h[1][1] else 0) for h in edges.values() if len(h) == 2]
        changed = True
        while changed:                                                   # the patches: the lowest face index spreads to a fixed point
            changed = False
            for a, b, _p in joined:
                low = min(patch[a], patch[b])
                if patch[a] != low or patch[b] != low:
                    patch[a] = patch[b] = low
                    changed = True
        s = {i: (0 if patch[i] == i else None) for i in corners}         # the parities: from the root outward, to a fixed point
        changed = True
        while changed:
            changed = False
            for a, b, p in joined:
                if s[a] is not None and s[b] is None:
                    s[b], changed = s[a] ^ p, True
                elif s[b] is not None and s[a] is None:
                    s[a], changed = s[b] ^ p, True
        roots = sorted(set(patch.values()))
        bad = {patch[a] for a, b, p in joined if s[a] ^ s[b] != p}
        own = {}                                                         # half-edges per (edge, patch)
        for e, h in edges.items():
            for i, _d in h:
                own[(e, patch[i])] = own.get((e, patch[i]), 0) + 1
        opened = {r for (e, r), n in own.items() if n != 2}
        members = {r: [i for i in corners if patch[i] == r] for r in roots}
        q = {}
        if outward and len(kept_vertices):
            box = v[kept_vertices]
            q = dict(zip(kept_vertices.tolist(), quantise_np(box, box.min(0), box.max(0))))
        stats["patches"], stats["patches_closed"], stats["patches_unorientable"] = len(roots), len(roots) - len(opened), len(bad)
        for r in roots:
            if r in bad:
                for i in members[r]:
                    s[i] = 0
                continue
            majority = True
            if outward and r not in opened:
                total = sum((-1 if s[i] else 1) * det_int(*(q[x] for x in corners[i])) for i in members[r])
                if total < 0:
                    stats["patches_inverted"] += 1
                    for i in members[r]:
                        s[i] ^= 1
                majority = total == 0
                stats["patches_undecided"] += total == 0
            if majority and 2 * sum(s[i] for i in members[r]) > len(members[r]):
                for i in members[r]:
                    s[i] ^= 1
        flip = s
    for i in corners:
        if flip[i]:
            fate[i] = KEPT_FLIPPED
    out_faces = np.array([[new[c[0]], new[c[2]], new[c[1]]] if flip[i] else [new[x] for x in c] for i, c in corners.items()],
                         dtype=np.int32).reshape(-1, 3)
    keyable = rep >= 0
    stats.update(vertices_out=len(kept_vertices), faces_out=len(live), vertices_welded=int((keyable & (rep != np.arange(nv))).sum()),
                 vertices_unkeyable=int((~keyable).sum()), faces_invalid=int((fate == INVALID).sum()), faces_unkeyable=int((fate == UNKEYABLE).sum()),
                 faces_collapsed=int((fate == COLLAPSED).sum()), faces_duplicate=int((fate == DUPLICATE).sum()),
                 faces_flipped=int((fate == KEPT_FLIPPED).sum()))
    stats["vertices_unreferenced"] = int((keyable & (rep == np.arange(nv))).sum()) - len(kept_vertices)
    stats = {k: int(stats[k]) for k in STATS}
    return {"vertices": v[kept_vertices], "faces": out_faces, "stats": stats, "vertex_map": vertex_map.astype(np.int32),
            "kept_vertices": kept_vertices.astype(np.int32), "face_map": live.astype(np.int32), "face_fate": fate,
            "face_patch": np.array([patch[int(i)] for i in live], dtype=np.int32), "rep": rep.astype(np.int32)}


def det_sum(vertices, faces):
    """six times the signed volume of a mesh on step 6's grid, a Python integer"""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    q = quantise_np(v, v.min(0), v.max(0))
    return sum(det_int(q[a], q[b], q[c]) for a, b, c in np.asarray(faces, dtype=np.int64).tolist())


def stats_row(stats):
    return [stats[k] for k in STATS]


def changed(stats):
    """what frame.read_mesh_repair adds"""
    return any(stats[k] for k in CHANGES)


# ---- the meshes

def explode(mesh):
    """a triangle soup: three private vertices per face"""
    v, f = mesh
    f = np.asarray(f, dtype=np.int64)
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32)[f.reshape(-1)]), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)


def flipped(mesh, which):
    """the faces `which` (indices or a mask) wound the other way: (a, b, c) -> (a, c, b)"""
    v, f = mesh
    f = np.array(f, dtype=np.int32)
    f[which] = f[which][:, [0, 2, 1]]
    return v, f


def ico(level, scale=1.0, shift=0.0):
    v, f = mm.icosphere(level)
    return (np.asarray(v, dtype=np.float64) * scale + shift).astype(np.float32), np.asarray(f, dtype=np.int32)


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]          # outward, counter-clockwise from outside
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.array(f, dtype=np.int32)


def signed_zero():
    """a tetrahedron soup on the origin whose odd copies carry -0.0 where the even ones carry +0.0"""
    v, f = explode(sm.tetrahedron())
    v = v.copy()
    odd = v[1::2]
    odd[odd == 0] = np.float32(-0.0)
    v[1::2] = odd
    assert np.signbit(v).any() and not (v < 0).any()
    return v, f


def nan_vertex():
    """two tetrahedra; vertex 5, of the second, is NaN: the three faces on it are unkeyable, the fourth is an open patch of its own"""
    tv, tf = sm.tetrahedron()
    v = np.concatenate([tv, tv + np.float32(3.0)]).astype(np.float32)
    v[5, 1] = np.nan
    return v, np.concatenate([tf, tf + 4]).astype(np.int32)


GRID_TOL = 0.5


def grid():
    """tol = 0.5: vertices 0 and 1 are tol / 4 apart either side of the wall x = 0.5 and stay apart; 2 and 3 share a cell and merge, so do
    7 and 8 in a cell of negative indices; 6 is beyond 2^62 cells and unkeyable"""
    v = [[0.49, 0.1, 0.1], [0.615, 0.1, 0.1], [1.1, 1.1, 1.1], [1.4, 1.3, 1.2], [2.1, 0.1, 0.1], [0.1, 2.1, 0.1], [3e18, 0.0, 0.0],
         [-0.2, -0.3, 0.1], [-0.4, -0.1, 0.2]]
    f = [[0, 1, 4], [2, 3, 5], [2, 4, 5], [3, 5, 4], [6, 4, 5], [7, 8, 4], [7, 4, 5], [8, 0, 5]]
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int32)


def crowd():
    """4 096 vertices: 64 points, 64 bit-equal copies of each, in shuffled order; 256 faces over members picked at random"""
    rng = np.random.default_rng(11)
    points = rng.uniform(-1.0, 1.0, (64, 3)).astype(np.float32)
    group = rng.permutation(np.repeat(np.arange(64), 64))
    members = [np.nonzero(group == g)[0] for g in range(64)]
    pick = lambda g: int(rng.choice(members[g % 64]))
    f = [[pick(g), pick(g + 1), pick(g + 2)] for _ in range(4) for g in range(64)]
    return points[group], np.array(f, dtype=np.int32), group


def strip(n=4500):
    """a consistently wound strip of n triangles as a soup, every third face flipped: more than 2 x 2 048 output vertices and faces"""
    pos = np.arange(n + 2)
    v = np.stack([pos * 0.5, pos % 2, 0.01 * pos], 1).astype(np.float32)
    i = np.arange(n)
    f = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1)).astype(np.int32)
    return explode(flipped((v, f), i % 3 == 1))


def bad_faces():
    """smooth_cases.bad_faces -- indices out of range, repeated corners, vertex 6 no face names -- and face 0 twice more: rotated, and
    wound the other way.  The lowest index, 0, survives"""
    v, f = sm.bad_faces()
    return v, np.concatenate([f, [[1, 2, 0], [0, 2, 1]]]).astype(np.int32)


def moebius(n=8):
    """a Moebius strip of 2 n triangles: two rows of n vertices, the last quad joined to the first with the rows swapped"""
    t = np.arange(n) * (2.0 * np.pi / n)
    ring = np.stack([np.cos(t), np.sin(t), np.zeros(n)], 1)
    off = 0.3 * np.stack([np.cos(t / 2) * np.cos(t), np.cos(t / 2) * np.sin(t), np.sin(t / 2)], 1)
    v = np.concatenate([ring + off, ring - off]).astype(np.float32)                  # top i, bottom n + i
    f = []
    for i in range(n):
        t0, b0 = i, n + i
        t1, b1 = (i + 1, n + i + 1) if i + 1 < n else (n, 0)                         # the twist
        f += [[t0, b0, t1], [b0, b1, t1]]
    return v, np.array(f, dtype=np.int32)


def sheet():
    v, f = sc.flat_sheet(n=3)
    return np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32)


def shared_edge():
    """two tetrahedra glued along the edge {0, 1}: four half-edges on it, two of each solid"""
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [0.5, 1, 0.5], [-1, 0, 0.5], [-0.5, -1, 0.5]], dtype=np.float32)

    def tetra(a, b, c, d):
        fs = [[a, b, c], [a, d, b], [b, d, c], [a, c, d]]
        vol = np.linalg.det(np.stack([v[b] - v[a], v[c] - v[a], v[d] - v[a]]).astype(np.float64))
        return fs if vol < 0 else [[x, z, y] for x, y, z in fs]                      # outward either way

    return v, np.array(tetra(0, 1, 2, 3) + tetra(0, 1, 4, 5), dtype=np.int32)


def nested():
    """a sphere inside a sphere, the inner wall facing inward: a solid with a cavity, wound as a solid's boundary is"""
    ov, of = ico(1, 2.0)
    iv, fi = ico(1, 0.75)
    return np.concatenate([ov, iv]), np.concatenate([of, fi[:, [0, 2, 1]] + len(ov)]).astype(np.int32)


def flat_closed():
    v, f = sm.one_triangle()
    f = np.asarray(f, dtype=np.int32).reshape(-1, 3)[:1]
    return np.asarray(v, dtype=np.float32), np.concatenate([f, f[:, [0, 2, 1]]])


@functools.lru_cache(maxsize=None)
def mc_sphere_clean():
    v, f = sc.mc_sphere()
    return np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32)


def mc_sphere_soup():
    """marching cubes' sphere exploded, a seeded half of its faces flipped, the faces shuffled"""
    v, f = mc_sphere_clean()
    rng = np.random.default_rng(21)
    half = rng.permutation(len(f))[:len(f) // 2]
    sv, sf = explode(flipped((v, f), half))
    return sv, np.ascontiguousarray(sf[rng.permutation(len(sf))])


SPHERE_FLIPS = np.random.default_rng(4).permutation(320)[:160]
_THIRD = np.arange(288) % 3 == 0
_ODD, _EVEN = np.arange(288) % 2 == 1, np.arange(288) % 2 == 0
ALL = dict(tol=0.0, weld=True, drop_duplicates=True, orient=True, outward=True)

# name -> (vertices, faces, repair_np's keywords)
CASES = {
    "cube_soup": lambda: (*explode(cube()), ALL),
    "signed_zero": lambda: (*signed_zero(), ALL),
    "nan_vertex": lambda: (*nan_vertex(), ALL),
    "grid": lambda: (*grid(), {**ALL, "tol": GRID_TOL}),
    "crowd": lambda: (*crowd()[:2], ALL),
    "strip": lambda: (*strip(), ALL),
    "bad_faces": lambda: (*bad_faces(), ALL),
    "flipped_sphere": lambda: (*flipped(ico(2), SPHERE_FLIPS), ALL),
    "inside_out": lambda: (*flipped(ico(1), slice(None)), ALL),
    "inside_out_not_outward": lambda: (*flipped(ico(1), slice(None)), {**ALL, "outward": False}),
    "moebius": lambda: (*moebius(), ALL),
    "open_sheet_third": lambda: (*flipped(sheet(), _THIRD), ALL),
    "open_sheet_half": lambda: (*flipped(sheet(), _ODD), ALL),
    "open_sheet_half_root_flipped": lambda: (*flipped(sheet(), _EVEN), ALL),
    "shared_edge": lambda: (*shared_edge(), ALL),
    "nested": lambda: (*nested(), ALL),
    "flat_closed": lambda: (*flat_closed(), {**ALL, "drop_duplicates": False}),
    "empty": lambda: (*sm.empty(), ALL),
    "no_faces": lambda: (*sm.no_faces(), ALL),
    "mc_sphere_soup": lambda: (*mc_sphere_soup(), ALL),
    "bad_faces_no_flags": lambda: (*bad_faces(), dict(tol=0.0, weld=False, drop_duplicates=False, orient=False, outward=False)),
    "mc_sphere_no_flags": lambda: (*mc_sphere_clean(), dict(tol=0.0, weld=False, drop_duplicates=False, orient=False, outward=False)),
}
# cases without duplicates or exact-half ties: a shuffled face order must change no bit of the vertex outputs or the stats
ORDER_FREE = ("cube_soup", "nan_vertex", "strip", "flipped_sphere", "moebius", "open_sheet_third", "shared_edge", "nested", "mc_sphere_soup")


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, keywords, the restatement's result); built once and left unchanged"""
    v, f, kw = CASES[name]()
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
    return v, f, dict(kw), repair_np(v, f, **kw)
