"""A numpy restatement of the quadric vertex clustering of csrc/gpnerf_simplify.hip (THE DEFINITION in include/gpnerf_hip.h, step by
step and operation by operation: float32 for step 1, float64 for steps 4 and 5, Python loops for the lists and groups), the meshes
the simplification tests run it on, and the bounds they check with."""
import functools
import math

import numpy as np

import mesh_cases
import mesh_metric_cases as mm

EPS = 1e-3
STATS = ("vertices_out", "faces_out", "faces_invalid", "faces_collapsed", "faces_cancelled", "faces_duplicate", "clusters_clamped",
         "clusters_dropped")


def vertex_cells(vertices, lo, cell, cells):
    """step 1: (q int64 [n,3], in_grid bool [n], linear index int64 [n], -1 outside)"""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    lo = np.asarray(lo, dtype=np.float32)
    cells = np.asarray(cells, dtype=np.int64)
    with np.errstate(all="ignore"):
        t = np.floor((v - lo[None, :]) / np.float32(cell))                  # float32 throughout
        ok = np.isfinite(v).all(1) & (t >= 0).all(1) & (t < cells[None, :].astype(np.float32)).all(1)
    q = np.where(ok[:, None], t, 0).astype(np.int64)
    lin = np.where(ok, (q[:, 0] * cells[1] + q[:, 1]) * cells[2] + q[:, 2], -1)
    return q, ok, lin


def face_terms(p0, p1, p2):
    """step 4's nine terms of one face (float64 scalars), or None for l == 0"""
    ax, ay, az = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
    bx, by, bz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
    nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
    l = np.sqrt((nx * nx + ny * ny) + nz * nz)
    if l == 0.0:
        return None
    ux, uy, uz = nx / l, ny / l, nz / l
    w = 0.5 * l
    d = -((ux * p0[0] + uy * p0[1]) + uz * p0[2])
    wx, wy, wz, wd = w * ux, w * uy, w * uz, w * d
    return np.array([wx * ux, wx * uy, wx * uz, wy * uy, wy * uz, wz * uz, wd * ux, wd * uy, wd * uz], dtype=np.float64)


def quadric_sum(terms):
    """THE ORDER OF THE SUM: 64 partials from 0, partial j adds entries j, j + 64, ...; the partials added in order"""
    partial = np.zeros((64, 9), dtype=np.float64)
    for j, t in enumerate(terms):
        if t is not None:
            partial[j % 64] = partial[j % 64] + t
    total = partial[0].copy()
    for j in range(1, 64):
        total = total + partial[j]
    return total


def cluster_position(q9, q, lo, cell):
    """step 5: (position float32 [3], clamped)"""
    Axx, Axy, Axz, Ayy, Ayz, Azz, bx, by, bz = (np.float64(x) for x in q9)
    lo = [np.float64(np.float32(x)) for x in lo]
    cell = np.float64(np.float32(cell))
    qd = [np.float64(int(k)) for k in q]
    c = [lo[k] + (qd[k] + 0.5) * cell for k in range(3)]
    blo = [lo[k] + qd[k] * cell for k in range(3)]
    bhi = [lo[k] + (qd[k] + 1.0) * cell for k in range(3)]
    x = list(c)
    lam = (1e-3 * ((Axx + Ayy) + Azz)) / 3.0
    if lam != 0.0:
        with np.errstate(all="ignore"):
            m00, m11, m22 = Axx + lam, Ayy + lam, Azz + lam
            r0 = ((Axx * c[0] + Axy * c[1]) + Axz * c[2]) + bx
            r1 = ((Axy * c[0] + Ayy * c[1]) + Ayz * c[2]) + by
            r2 = ((Axz * c[0] + Ayz * c[1]) + Azz * c[2]) + bz
            l00 = np.sqrt(m00)
            l10, l20 = Axy / l00, Axz / l00
            l11 = np.sqrt(m11 - l10 * l10)
            l21 = (Ayz - l20 * l10) / l11
            l22 = np.sqrt((m22 - l20 * l20) - l21 * l21)
            y0 = r0 / l00
            y1 = (r1 - l10 * y0) / l11
            y2 = ((r2 - l20 * y0) - l21 * y1) / l22
            s2 = y2 / l22
            s1 = (y1 - l21 * s2) / l11
            s0 = ((y0 - l10 * s1) - l20 * s2) / l00
            t = [c[0] - s0, c[1] - s1, c[2] - s2]
        if all(np.isfinite(v) for v in t):
            x = t
    out, moved = [], False
    for k in range(3):
        y = blo[k] if x[k] < blo[k] else (bhi[k] if x[k] > bhi[k] else x[k])
        moved = moved or y != x[k]
        out.append(np.float32(y))
    return np.array(out, dtype=np.float32), moved


def _sorted_parity(ids):
    a, b, c = (int(i) for i in ids)
    parity = 1
    if a > b:
        a, b, parity = b, a, -parity
    if b > c:
        b, c, parity = c, b, -parity
    if a > b:
        a, b, parity = b, a, -parity
    return (a, b, c), parity


def simplify_np(vertices, faces, lo, cell, cells):
    """{"vertices" float32 [n,3], "faces" int32 [m,3], "vertex_map" int32 [n_v], "stats" dict, "positions"/"cluster_of" for the bound}"""
    v32 = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    nv, nf = len(v32), len(f)
    cells = [int(c) for c in cells]
    q, ok, lin = vertex_cells(v32, lo, cell, cells)
    in_range = ((f >= 0) & (f < nv)).all(1) if nf else np.zeros(0, dtype=bool)
    safe = np.where(in_range[:, None], f, 0)
    valid = in_range & (ok[safe].all(1) if nv else False)
    # step 3
    occupied = np.unique(lin[f[valid]].reshape(-1)) if valid.any() else np.zeros(0, dtype=np.int64)
    cluster_of_cell = {int(c): i for i, c in enumerate(occupied)}
    fclu = np.full((nf, 3), -1, dtype=np.int64)
    for i in np.nonzero(valid)[0]:
        fclu[i] = [cluster_of_cell[int(lin[j])] for j in f[i]]
    # step 4: the lists, ascending by construction
    lists = [[] for _ in occupied]
    for i in np.nonzero(valid)[0]:
        seen = []
        for c in fclu[i]:
            if c not in seen:
                seen.append(c)
                lists[c].append(int(i))
    v64 = v32.astype(np.float64)
    terms = {int(i): face_terms(v64[f[i, 0]], v64[f[i, 1]], v64[f[i, 2]]) for i in np.nonzero(valid)[0]}
    positions = np.zeros((len(occupied), 3), dtype=np.float32)
    clamped = 0
    for c, cell_index in enumerate(occupied):
        q9 = quadric_sum([terms[i] for i in lists[c]])
        qc = (int(cell_index) // (cells[1] * cells[2]), (int(cell_index) // cells[2]) % cells[1], int(cell_index) % cells[2])
        positions[c], moved = cluster_position(q9, qc, lo, cell)
        clamped += bool(moved)
    # step 6
    collapsed = 0
    groups = {}
    for i in np.nonzero(valid)[0]:
        a, b, c = fclu[i]
        if a == b or b == c or a == c:
            collapsed += 1
            continue
        key, parity = _sorted_parity(fclu[i])
        groups.setdefault(key, []).append((int(i), parity))
    kept, cancelled, duplicate = [], 0, 0
    for members in groups.values():
        pos = [i for i, p in members if p > 0]
        neg = [i for i, p in members if p < 0]
        net = len(pos) - len(neg)
        cancelled += 2 * min(len(pos), len(neg))
        if net != 0:
            kept.append(min(pos if net > 0 else neg))
            duplicate += abs(net) - 1
    kept.sort()
    # step 7
    used = np.zeros(len(occupied), dtype=bool)
    for i in kept:
        used[fclu[i]] = True
    number = np.where(used, np.cumsum(used) - 1, -1)
    out_faces = np.array([[number[c] for c in fclu[i]] for i in kept], dtype=np.int32).reshape(-1, 3)
    vertex_map = np.full(nv, -1, dtype=np.int32)
    cluster_of_vertex = np.full(nv, -1, dtype=np.int64)
    for j in range(nv):
        if ok[j] and int(lin[j]) in cluster_of_cell:
            cluster_of_vertex[j] = cluster_of_cell[int(lin[j])]
            vertex_map[j] = number[cluster_of_vertex[j]]
    stats = dict(zip(STATS, (int(used.sum()), len(kept), int(nf - valid.sum()), collapsed, cancelled, duplicate, clamped,
                             int(len(occupied) - used.sum()))))
    return {"vertices": positions[used], "faces": out_faces, "vertex_map": vertex_map, "stats": stats, "positions": positions,
            "cluster_of": cluster_of_vertex, "valid": valid}


def stats_row(stats):
    return [stats[k] for k in STATS]


def auto_grid(vertices, cell):
    """the box rule of frame.simplify_mesh and of the issue's checks: lo = floor(min) - cell / 4 ... here with the checks' literal
    0.25: lo = floor(min) - 0.25, cells = ceil((max - lo) / cell) + 1"""
    v = np.asarray(vertices, dtype=np.float64)
    lo = np.floor(v.min(0)) - 0.25
    cells = np.ceil((v.max(0) - lo) / cell).astype(np.int64) + 1
    return lo.astype(np.float32), [int(c) for c in cells]


def distance_bound_ok(vertices, faces, res, cell, lo, cells):
    """the derived guarantee: every vertex of a valid face within sqrt(3) cell of its cluster's position, plus float32 ulps of the
    coordinates' range.  Returns the largest distance in cells."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    idx = np.unique(f[res["valid"]].reshape(-1)) if res["valid"].any() else np.zeros(0, dtype=np.int64)
    if not len(idx):
        return 0.0
    d = np.linalg.norm(v[idx] - res["positions"][res["cluster_of"][idx]].astype(np.float64), axis=1)
    span = float(np.abs(np.asarray(lo, dtype=np.float64)).max() + max(cells) * cell)
    assert d.max() <= math.sqrt(3.0) * cell + 8 * 2.0 ** -23 * span, (d.max(), cell)
    return float(d.max() / cell)


def position_tolerance(x, lo, cell, cells):
    """one float32 ulp per coordinate: 2^-23 max(|x|, |lo| + cells cell)"""
    span = np.abs(np.asarray(lo, dtype=np.float64)) + np.asarray(cells, dtype=np.float64) * float(cell)
    return 2.0 ** -23 * np.maximum(np.abs(np.asarray(x, dtype=np.float64)), span[None, :])


# ---- the meshes

@functools.lru_cache(maxsize=None)
def mc_sphere():
    v, f = mesh_cases.marching_cubes_np(mesh_cases.sphere_field(32, 10.0), 0.02)
    return v, f.astype(np.int32)


@functools.lru_cache(maxsize=None)
def mc_torus():
    v, f = mesh_cases.marching_cubes_np(mesh_cases.torus_field(48, 13.0, 5.0), 0.02)
    return v, f.astype(np.int32)


@functools.lru_cache(maxsize=None)
def ico5():
    v, f = mm.icosphere(3)
    return (np.asarray(v, dtype=np.float64) * 5.0).astype(np.float32), np.asarray(f, dtype=np.int32)


def one_triangle():
    """corners in three cells of a grid of unit cells from (0, 0, 0)"""
    return np.array([[0.3, 0.4, 0.5], [1.6, 0.2, 0.4], [0.5, 1.7, 0.6]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def coincident(orientations):
    """triangles over three cells, one per entry of `orientations` (+1: corner order 0 1 2 of its own three vertices, -1: 0 2 1); the
    vertices of each differ slightly, the cells do not"""
    base = one_triangle()[0].astype(np.float64)
    v, f = [], []
    for i, o in enumerate(orientations):
        v.append(base + 0.01 * (i + 1))
        f.append([3 * i, 3 * i + 1, 3 * i + 2] if o > 0 else [3 * i, 3 * i + 2, 3 * i + 1])
    return np.concatenate(v).astype(np.float32), np.array(f, dtype=np.int32)


def bad_faces():
    """a good triangle, then: a bad index (too large, negative), a NaN vertex, a vertex outside the grid on each of the six sides, and
    a zero-area face across three cells (collinear corners), in a grid of 4 x 4 x 4 unit cells from (0, 0, 0)"""
    v = [[0.3, 0.4, 0.5], [1.6, 0.2, 0.4], [0.5, 1.7, 0.6],          # 0-2: good
         [np.nan, 0.5, 0.5],                                       # 3
         [-0.1, 0.5, 0.5], [4.1, 0.5, 0.5], [0.5, -0.1, 0.5], [0.5, 4.0, 0.5], [0.5, 0.5, -2.0], [0.5, 0.5, 7.0],   # 4-9: outside
         [0.5, 2.5, 2.5], [1.5, 2.5, 2.5], [2.5, 2.5, 2.5],          # 10-12: collinear
         [np.inf, 0.5, 0.5]]                                       # 13
    f = [[0, 1, 2], [0, 1, 14], [0, -1, 2], [0, 1, 3]] + [[0, 1, k] for k in range(4, 10)] + [[10, 11, 12], [13, 1, 2]]
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int32)


def flat_sheet(n=9, h=1.3, cell=1.0):
    """z = h over n x n cells of edge `cell` from (0, 0, 0): a regular grid of vertices four per cell edge, two triangles per square"""
    m = 4 * n + 1
    xs = (np.arange(m) * (cell / 4.0)).astype(np.float64)
    gx, gy = np.meshgrid(xs, xs, indexing="ij")
    inside = 1e-3 * cell
    v = np.stack([np.clip(gx, inside, n * cell - inside), np.clip(gy, inside, n * cell - inside), np.full_like(gx, h)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(m - 1), np.arange(m - 1), indexing="ij")
    a, b, c, d = (i * m + j).ravel(), ((i + 1) * m + j).ravel(), ((i + 1) * m + j + 1).ravel(), (i * m + j + 1).ravel()
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return v.astype(np.float32), f.astype(np.int32)


def fan(n=3000, seed=0, shuffled=False):
    """n triangles around one vertex in the middle of cell (2, 2, 2) of a 5 x 5 x 5 grid of unit cells from (0, 0, 0); the rim, n + 1
    points on a circle of radius 1.4 tilted out of the plane, lies in other cells: the centre's cluster has all n faces"""
    t = np.linspace(0.0, 2.0 * np.pi, n + 1, endpoint=False)
    rim = np.stack([2.5 + 1.4 * np.cos(t), 2.5 + 1.4 * np.sin(t), 2.5 + 0.9 * np.sin(3 * t)], 1)
    v = np.concatenate([[[2.5, 2.5, 2.5]], rim]).astype(np.float32)
    f = np.stack([np.zeros(n, dtype=np.int64), 1 + np.arange(n), 2 + np.arange(n)], 1).astype(np.int32)
    if shuffled:
        f = f[np.random.default_rng(seed).permutation(n)]
    return v, f
