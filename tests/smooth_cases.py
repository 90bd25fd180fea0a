"""A numpy restatement of the mesh adjacency, the topology counts and the Taubin smoothing of csrc/gpnerf_meshtopo.hip (THE DEFINITION
in include/gpnerf_hip.h, step by step and operation by operation: Python loops over faces and half-edges for the edges and the CSR,
float64 adds in ascending neighbour order for the passes), the meshes the tests run it on, and the two figures of the smoothing's
property test (the mean angle between face normals and the radial direction, the enclosed volume)."""
import functools

import numpy as np

import mesh_cases
import simplify_cases as sc

STATS = ("faces_used", "faces_dropped", "vertices_referenced", "edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "euler",
         "boundary_vertices", "max_valence")
REFERENCED, BOUNDARY = 1, 2
LAM, MU, ITERATIONS = 0.5, -0.53, 10
LONG_LIST = 32                                     # smooth_pass_np walks longer neighbour lists one by one


def usable_faces(faces, n_vertices):
    """step 1: bool [m] -- three indices in [0, n_vertices), pairwise distinct"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < n_vertices)).all(1)
    return ok & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def edges_np(faces, n_vertices):
    """step 2: {(lo, hi): [fwd, bwd]} over the half-edges of the usable faces"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    edges = {}
    for i in np.nonzero(usable_faces(f, n_vertices))[0]:
        a, b, c = (int(x) for x in f[i])
        for p, q in ((a, b), (b, c), (c, a)):
            e = edges.setdefault((min(p, q), max(p, q)), [0, 0])
            e[0 if p < q else 1] += 1
    return edges


def adjacency_np(faces, n_vertices):
    """steps 3 and 4: {"stats": dict, "start" int64 [n + 1], "neighbours" int32 [start[n]], "vertex_flags" uint8 [n]}"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = int(n_vertices)
    ok = usable_faces(f, n)
    edges = edges_np(f, n)
    flags = np.zeros(n, dtype=np.uint8)
    flags[np.unique(f[ok].reshape(-1))] |= REFERENCED
    lists = [[] for _ in range(n)]
    boundary = nonmanifold = inconsistent = 0
    for (lo, hi), (fwd, bwd) in edges.items():
        m = fwd + bwd
        lists[lo].append(hi)
        lists[hi].append(lo)
        boundary += m == 1
        nonmanifold += m >= 3
        inconsistent += m == 2 and fwd != bwd
        if m == 1 or m >= 3:
            flags[lo] |= BOUNDARY
            flags[hi] |= BOUNDARY
    start = np.zeros(n + 1, dtype=np.int64)
    for v in range(n):
        lists[v].sort()
        start[v + 1] = start[v] + len(lists[v])
    neighbours = np.array([j for l in lists for j in l], dtype=np.int32)
    used, referenced = int(ok.sum()), int((flags & REFERENCED != 0).sum())
    stats = dict(zip(STATS, (used, int(len(f) - used), referenced, len(edges), int(boundary), int(nonmanifold), int(inconsistent),
                             referenced - len(edges) + used, int((flags & BOUNDARY != 0).sum()), max([len(l) for l in lists], default=0))))
    return {"stats": stats, "start": start, "neighbours": neighbours, "vertex_flags": flags}


def stats_row(stats):
    return [stats[k] for k in STATS]


def read_topology(stats):
    """what frame.read_mesh_topology adds"""
    closed = stats["boundary_edges"] == 0 and stats["nonmanifold_edges"] == 0
    oriented = stats["inconsistent_edges"] == 0 and stats["nonmanifold_edges"] == 0
    return {**stats, "closed": closed, "oriented": oriented, "watertight": closed and oriented}


def smooth_pass_np(x32, adj, t, pin_boundary=True):
    """step 5, one Jacobi pass with factor t on float32 positions [n,3]: s = 0.0; s = s + x_j over the neighbours in ascending index --
    done for all vertices at once, neighbour rank by neighbour rank, which is each vertex's own ascending order; lists beyond LONG_LIST
    one vertex at a time --; x' = float32(x + t
    (s / k - x)), float64 throughout; vertices without a neighbour, and pinned ones, are copied"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32).reshape(-1, 3)
    start, nb = adj["start"], adj["neighbours"].astype(np.int64)
    k = np.diff(start)
    moves = k >= 1
    if pin_boundary:
        moves &= (adj["vertex_flags"] & BOUNDARY) == 0
    out = x32.copy()
    idx = np.nonzero(moves)[0]
    if not len(idx):
        return out
    x = x32.astype(np.float64)
    s = np.zeros((len(idx), 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        few = k[idx] <= LONG_LIST
        for r in range(int(k[idx][few].max()) if few.any() else 0):
            has = few & (k[idx] > r)
            s[has] = s[has] + x[nb[start[idx[has]] + r]]
        for row in np.nonzero(~few)[0]:                                   # a long list: numpy's accumulate adds one after the other too
            i = idx[row]
            s[row] = np.add.accumulate(np.concatenate([np.zeros((1, 3)), x[nb[start[i]:start[i + 1]]]]), axis=0)[-1]
        xi = x[idx]
        out[idx] = (xi + np.float64(t) * (s / k[idx].astype(np.float64)[:, None] - xi)).astype(np.float32)
    return out


def smooth_np(vertices, adj, iterations=ITERATIONS, lam=LAM, mu=MU, pin_boundary=True):
    x = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3).copy()
    for _ in range(int(iterations)):
        x = smooth_pass_np(x, adj, lam, pin_boundary)
        x = smooth_pass_np(x, adj, mu, pin_boundary)
    return x


# ---- the property's two figures

def normal_angle_deg(vertices, faces, centre):
    """the mean over the faces (those with an area) of the angle between the face normal and the direction from `centre` to the
    face's centroid, in degrees"""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    l = np.linalg.norm(n, axis=1)
    r = (a + b + c) / 3.0 - np.asarray(centre, dtype=np.float64)
    keep = l > 0
    cos = np.sum(n[keep] * r[keep], axis=1) / (l[keep] * np.linalg.norm(r[keep], axis=1))
    return float(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))).mean())


def enclosed_volume(vertices, faces):
    """|sum over the faces of det(a, b, c) / 6| (a closed, oriented mesh)"""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    return float(abs(np.sum(a * np.cross(b, c)) / 6.0))


# ---- the meshes

SPHERE_CENTRE = np.array([15.5 + 0.31, 15.5 - 0.17, 15.5 + 0.07])       # mesh_cases.sphere_field(32, .)'s


@functools.lru_cache(maxsize=None)
def binary_sphere():
    """marching cubes at 0.02 on a BINARY field (0.04 within 10 of sphere_field's off-lattice centre of a 32^3 cube, 0 elsewhere): every
    vertex at the middle of a lattice edge, the staircase the smoothing is for"""
    g = np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing="ij"), -1).astype(np.float64)
    field = np.where(np.linalg.norm(g - SPHERE_CENTRE, axis=-1) < 10.0, 0.04, 0.0).astype(np.float32)
    v, f = mesh_cases.marching_cubes_np(field, 0.02)
    return np.asarray(v, dtype=np.float32), f.astype(np.int32)


def empty():
    return np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)


def no_faces():
    """vertices without a face: nothing referenced, nothing moves"""
    return np.arange(15, dtype=np.float32).reshape(5, 3), np.zeros((0, 3), dtype=np.int32)


def one_triangle():
    return sc.one_triangle()


_QUAD = np.array([[0.0, 0.0, 0.1], [1.0, 0.1, 0.0], [1.1, 1.0, 0.3], [0.1, 0.9, -0.2]], dtype=np.float32)


def two_triangles(flipped=False):
    """two triangles on the edge {0, 2}: used once in each direction, or -- the second triangle flipped -- twice in one"""
    return _QUAD.copy(), np.array([[0, 1, 2], [0, 3, 2] if flipped else [0, 2, 3]], dtype=np.int32)


def three_on_an_edge():
    """three triangles on the edge {0, 1}: non-manifold"""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.5, -0.5, 0.9], [0.5, -0.5, -0.9]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], dtype=np.int32)


def bad_faces():
    """two good triangles, then an index that is too large, one that equals n_vertices, a negative one, a repeated one (twice), and
    vertex 6 that no face names while vertex 5 is named by dropped faces only"""
    v = np.concatenate([_QUAD, [[2.0, 0.5, 0.4], [3.0, 3.0, 3.0], [4.0, 4.0, 4.0]]]).astype(np.float32)
    f = [[0, 1, 2], [0, 2, 3], [0, 1, 99], [1, 2, 7], [0, -1, 2], [1, 1, 4], [5, 2, 5], [2, 1, 4]]
    return v, np.array(f, dtype=np.int32)


def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)


def bumpy_sheet():
    """simplify_cases.flat_sheet with a height that varies, so that a free border visibly moves and a pinned one visibly does not"""
    v, f = sc.flat_sheet()
    v = v.copy()
    v[:, 2] += (0.2 * np.sin(1.7 * v[:, 0].astype(np.float64)) * np.cos(2.3 * v[:, 1].astype(np.float64))).astype(np.float32)
    return v, f


def shuffled(mesh, seed=1):
    v, f = mesh
    return v, np.ascontiguousarray(f[np.random.default_rng(seed).permutation(len(f))])


# name -> (mesh, pin_boundary)
CASES = {
    "empty": lambda: (empty(), True),
    "no_faces": lambda: (no_faces(), True),
    "triangle_pinned": lambda: (one_triangle(), True),
    "triangle_free": lambda: (one_triangle(), False),
    "two_consistent": lambda: (two_triangles(), False),
    "two_flipped": lambda: (two_triangles(flipped=True), False),
    "three_on_an_edge": lambda: (three_on_an_edge(), True),
    "three_on_an_edge_free": lambda: (three_on_an_edge(), False),
    "bad_faces": lambda: (bad_faces(), False),
    "tetrahedron": lambda: (tetrahedron(), True),
    "mc_sphere": lambda: (sc.mc_sphere(), True),
    "mc_torus": lambda: (sc.mc_torus(), True),
    "ico5": lambda: (sc.ico5(), True),
    "flat_sheet_pinned": lambda: (sc.flat_sheet(), True),
    "flat_sheet_free": lambda: (sc.flat_sheet(), False),
    "sheet_pinned": lambda: (bumpy_sheet(), True),
    "sheet_free": lambda: (bumpy_sheet(), False),
    "fan": lambda: (sc.fan(3000), False),
    "fan_shuffled": lambda: (sc.fan(3000, shuffled=True), False),
    "binary_sphere": lambda: (binary_sphere(), True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, pin_boundary, the restatement's adjacency, its vertices after 1 iteration, after 10); built once and left
    unchanged"""
    (v, f), pin = CASES[name]()
    adj = adjacency_np(f, len(v))
    return v, f, pin, adj, smooth_np(v, adj, 1, pin_boundary=pin), smooth_np(v, adj, ITERATIONS, pin_boundary=pin)
