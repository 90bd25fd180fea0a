"""A numpy restatement of the mesh's connected components of csrc/gpnerf_meshcomp.hip (THE DEFINITION in include/gpnerf_hip.h,
operation by operation: the labels by a plain loop of minimum-label propagation over the usable faces to a fixed point, the numbering,
the table from the adjacency restatement's degrees and flags, the stats, the selection and the emitted mesh) and the meshes the tests
run it on."""
import functools

import numpy as np

import mesh_cases
import simplify_cases as sc
import smooth_cases as sm

STATS = ("components", "closed_components", "largest", "largest_faces", "largest_vertices", "largest_euler", "kept_components",
         "kept_vertices", "kept_faces")
COLS = ("label", "vertices", "edges", "faces", "euler", "boundary_vertices")
KEEP_ALL, KEEP_LARGEST, KEEP_MIN_FACES = range(3)


def labels_np(faces, n_vertices):
    """steps 1 - 3: label[v] = the smallest vertex index of v's component of the graph of the usable faces' edges, -1 for a vertex no
    usable face references.  Every referenced vertex starts with its own index; every sweep gives the three corners of every usable
    face the smallest of their three labels; the loop ends with the sweep that changes nothing."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[sm.usable_faces(f, n_vertices)]
    label = np.full(int(n_vertices), -1, dtype=np.int64)
    label[f.reshape(-1)] = f.reshape(-1)
    while len(f):
        low = label[f].min(axis=1)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, f[:, k], low)
        if np.array_equal(new, label):
            break
        label = new
    return label.astype(np.int32)


def components_np(faces, n_vertices, keep=KEEP_ALL, min_faces=1, adjacency=None, label=None):
    """steps 3 - 6: {"label", "vertex_component", "face_component" int32; "table" int64 [C, 6]; "stats" dict; "kept_vertices" (new -> old),
    "vertex_map" (old -> new or -1) int32; "kept_faces" (the original indices of the kept faces); "out_faces" int32 [m', 3]}"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = int(n_vertices)
    adj = adjacency if adjacency is not None else sm.adjacency_np(f, n)
    ok = sm.usable_faces(f, n)
    label = labels_np(f, n) if label is None else label
    roots = np.unique(label[label >= 0])                                  # ascending label: the numbering
    vcomp = np.full(n, -1, dtype=np.int32)
    vcomp[label >= 0] = np.searchsorted(roots, label[label >= 0])
    fcomp = np.full(len(f), -1, dtype=np.int32)
    fcomp[ok] = vcomp[f[ok, 0]]
    degree = np.diff(adj["start"])
    table = np.zeros((len(roots), len(COLS)), dtype=np.int64)
    for c, root in enumerate(roots):
        mine = vcomp == c
        v, twice, nf = int(mine.sum()), int(degree[mine].sum()), int((fcomp == c).sum())
        assert twice % 2 == 0
        table[c] = (root, v, twice // 2, nf, v - twice // 2 + nf, int(((adj["vertex_flags"][mine] & sm.BOUNDARY) != 0).sum()))
    largest = -1
    for c in range(len(roots)):                                           # the most faces; a tie goes to the lower number
        if largest < 0 or table[c, 3] > table[largest, 3]:
            largest = c
    if keep == KEEP_ALL:
        kept = np.ones(len(roots), dtype=bool)
    elif keep == KEEP_LARGEST:
        kept = np.arange(len(roots)) == largest
    else:
        kept = table[:, 3] >= min_faces
    vkeep = (vcomp >= 0) & kept[np.maximum(vcomp, 0)] if len(roots) else np.zeros(n, dtype=bool)
    fkeep = (fcomp >= 0) & kept[np.maximum(fcomp, 0)] if len(roots) else np.zeros(len(f), dtype=bool)
    kept_vertices = np.nonzero(vkeep)[0].astype(np.int32)
    vertex_map = np.full(n, -1, dtype=np.int32)
    vertex_map[kept_vertices] = np.arange(len(kept_vertices), dtype=np.int32)
    kept_faces = np.nonzero(fkeep)[0]
    out_faces = vertex_map[f[kept_faces]].astype(np.int32).reshape(-1, 3)
    stats = dict(zip(STATS, (len(roots), int((table[:, 5] == 0).sum()), largest,
                             *((int(table[largest, 3]), int(table[largest, 1]), int(table[largest, 4])) if largest >= 0 else (0, 0, 0)),
                             int(kept.sum()), len(kept_vertices), len(kept_faces))))
    return {"label": label, "vertex_component": vcomp, "face_component": fcomp, "table": table, "stats": stats, "kept_vertices": kept_vertices,
            "vertex_map": vertex_map, "kept_faces": kept_faces, "out_faces": out_faces}


def stats_row(stats):
    return [stats[k] for k in STATS]


def genus_np(row, inconsistent_edges, nonmanifold_edges):
    """what frame.read_mesh_components adds to a table row: (closed, genus or None)"""
    closed = int(row[5]) == 0
    euler = int(row[4])
    return closed, ((2 - euler) // 2 if closed and inconsistent_edges == 0 and nonmanifold_edges == 0 and euler % 2 == 0 else None)


# ---- the meshes

def bow_tie():
    """two triangles that share vertex 2 and no edge: ONE component under vertex connectivity"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0, 2, 0.5], [1, 2, -0.5]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)


def two_tetrahedra(shuffled=False):
    """two disjoint tetrahedra, the first on the even vertices 0 2 4 6 and the second on the odd 1 3 5 7 (labels 0 and 1), and vertex 8
    that no face names"""
    tv, tf = sm.tetrahedron()
    v = np.zeros((9, 3), dtype=np.float32)
    v[0:8:2], v[1:8:2], v[8] = tv, tv + np.float32(3.0), (9.0, 9.0, 9.0)
    f = np.concatenate([2 * tf, 2 * tf + 1]).astype(np.int32)
    if shuffled:
        f = np.ascontiguousarray(f[np.random.default_rng(5).permutation(len(f))])
    return v, f


def bit_reversed_strip(n=4096):
    """a strip of n triangles (i, i + 1, i + 2) along n + 2 positions whose vertex indices follow the bit-reversed order of the
    positions: neighbours along the strip are far apart in index, so the union-find's paths are long and cross workgroups"""
    bits = int(np.ceil(np.log2(n + 2)))
    pos = np.arange(n + 2)
    rev = np.zeros(n + 2, dtype=np.int64)
    for b in range(bits):
        rev |= ((pos >> b) & 1) << (bits - 1 - b)
    index = np.argsort(np.argsort(rev))                                  # position -> vertex index, a permutation of 0 .. n + 1
    v = np.zeros((n + 2, 3), dtype=np.float32)
    v[index] = np.stack([pos * 0.5, pos % 2, np.zeros(n + 2)], 1).astype(np.float32)
    f = np.stack([index[:-2], index[1:-1], index[2:]], 1).astype(np.int32)
    return v, f


def hub_last_fan(n=3000):
    """simplify_cases.fan(n) relabelled so that the hub has the HIGHEST index: every face's link lands on the hub's word"""
    v, f = sc.fan(n)
    nv = len(v)
    new = np.concatenate([[nv - 1], np.arange(nv - 1)])                  # old -> new: the hub goes last, the rim moves down by one
    out = np.zeros_like(v)
    out[new] = v
    return out, new[f.astype(np.int64)].astype(np.int32)


def ball_field(shape, centre, r):
    """mesh_cases.sphere_field's fall-off around `centre`: 0.02 at distance r, linear over 4 cells either side"""
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).astype(np.float64)
    d = np.linalg.norm(g - np.asarray(centre, dtype=np.float64), axis=-1)
    return (np.clip(0.5 - (d - r) / 8.0, 0.0, 1.0) * 0.04).astype(np.float32)


def shell_field(shape, centre, r_in, r_out):
    """the same fall-off either side of a hollow shell: above 0.02 between the two radii"""
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).astype(np.float64)
    d = np.linalg.norm(g - np.asarray(centre, dtype=np.float64), axis=-1)
    mid, half = 0.5 * (r_in + r_out), 0.5 * (r_out - r_in)
    return (np.clip(0.5 - (np.abs(d - mid) - half) / 8.0, 0.0, 1.0) * 0.04).astype(np.float32)


SCENE_ISO = 0.02


@functools.lru_cache(maxsize=None)
def scene():
    """marching cubes at 0.02 on a 48^3 field, the maximum of: mesh_cases.torus_field(48, 12, 4); two identical balls of radius 4 an
    integer translation (32 steps in z) apart; a ball of radius 3; a ball of radius 1.5 (the smallest piece); and a hollow shell
    (radii 2.5 and 5) in the torus' hole, whose inner and outer surfaces are two components.  Seven closed components; tests/
    test_components_host.py holds the numbers."""
    shape = (48, 48, 48)
    field = mesh_cases.torus_field(48, 12.0, 4.0)
    for centre, r in (((8.31, 8.17, 8.07), 4.0), ((8.31, 8.17, 40.07), 4.0), ((40.2, 8.3, 40.1), 3.0), ((40.3, 40.2, 8.4), 1.5)):
        field = np.maximum(field, ball_field(shape, centre, r))
    field = np.maximum(field, shell_field(shape, (23.73, 23.73, 23.73), 2.5, 5.0))
    v, f = mesh_cases.marching_cubes_np(field, SCENE_ISO)
    return np.asarray(v, dtype=np.float32), f.astype(np.int32)


@functools.lru_cache(maxsize=None)
def noise_surface():
    """mesh_cases.all_cases_field()'s surface: not closed as a manifold, not oriented, hundreds of components -- the non-manifold stress"""
    v, f = mesh_cases.marching_cubes_np(mesh_cases.all_cases_field(), 0.02)
    return np.asarray(v, dtype=np.float32), f.astype(np.int32)


@functools.lru_cache(maxsize=None)
def twin_blobs():
    """two identical balls an integer translation (20 steps in z) apart: the same number of faces, a tie for the largest"""
    shape = (20, 20, 40)
    field = np.maximum(ball_field(shape, (9.31, 9.17, 9.07), 5.0), ball_field(shape, (9.31, 9.17, 29.07), 5.0))
    v, f = mesh_cases.marching_cubes_np(field, 0.02)
    return np.asarray(v, dtype=np.float32), f.astype(np.int32)


HAND_CASES = {
    "empty": sm.empty, "no_faces": sm.no_faces, "triangle": sm.one_triangle, "two_consistent": sm.two_triangles,
    "two_flipped": lambda: sm.two_triangles(flipped=True), "three_on_an_edge": sm.three_on_an_edge, "bad_faces": sm.bad_faces,
    "tetrahedron": sm.tetrahedron,
}
CASES = {
    **HAND_CASES,
    "bow_tie": bow_tie,
    "two_tetrahedra": two_tetrahedra,
    "two_tetrahedra_shuffled": lambda: two_tetrahedra(shuffled=True),
    "strip": bit_reversed_strip,
    "hub_last_fan": hub_last_fan,
    "scene": scene,
    "scene_shuffled": lambda: sm.shuffled(scene(), seed=3),
    "noise": noise_surface,
    "twin_blobs": twin_blobs,
}


@functools.lru_cache(maxsize=None)
def mesh(name):
    v, f = CASES[name]()
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def adjacency(name):
    v, f = mesh(name)
    return sm.adjacency_np(f, len(v))


@functools.lru_cache(maxsize=None)
def labels(name):
    v, f = mesh(name)
    return labels_np(f, len(v))


@functools.lru_cache(maxsize=None)
def case(name, keep=KEEP_ALL, min_faces=1):
    """(vertices, faces, the restatement's result for this selection); built once and left unchanged"""
    v, f = mesh(name)
    return v, f, components_np(f, len(v), keep, min_faces, adjacency=adjacency(name), label=labels(name))
