"""Meshes, query sets and the numpy restatements for the mesh-evaluation tests (gpnerf_meshdist.hip; include/gpnerf_hip.h states the
definitions restated here).

`closest_on_triangle(p, a, b, c, dtype)` is THE DISTANCE of the header, operation for operation, vectorised: run in float64 it is the
reference (a brute force over all faces, `nearest`), run in float32 on the same float32-rounded inputs it is the yardstick of the
tolerance rule: bound = 4 x the largest float32-vs-float64 difference of the per-query result, and at least
2^-22 max(1, max |coordinate|).  Nothing here looks at what the kernels give.
"""
import functools

import numpy as np

REGIONS = ("degenerate", "vertex_a", "vertex_b", "edge_ab", "vertex_c", "edge_ca", "edge_bc", "interior")


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _segment(a, e):
    """closest point of a + t e, t in [0, 1], to the origin"""
    ee = _dot(e, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0, np.clip(-_dot(a, e) / ee, 0, 1), 0).astype(a.dtype)
    return a + e * t[..., None]


def closest_on_triangle(p, a, b, c, dtype=np.float64):
    """(closest point RELATIVE to p, distance, region index into REGIONS); p, a, b, c broadcast to [..., 3]"""
    p, a, b, c = (np.asarray(x).astype(np.float32).astype(dtype) for x in (p, a, b, c))
    a, b, c = a - p, b - p, c - p
    ab, ac, bc = b - a, c - a, c - b
    n = _cross(ab, ac)
    nn = _dot(n, n)
    d1, d2 = -_dot(ab, a), -_dot(ac, a)
    d3, d4 = -_dot(ab, b), -_dot(ac, b)
    d5, d6 = -_dot(ab, c), -_dot(ac, c)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    den = (va + vb) + vc
    s_ab, s_bc, s_ca = _segment(a, ab), _segment(b, bc), _segment(a, ac)
    with np.errstate(divide="ignore", invalid="ignore"):
        v, w = vb / den, vc / den
        inner = (a + ab * v[..., None]) + ac * w[..., None]
    q0, q1, q2 = _dot(s_ab, s_ab), _dot(s_bc, s_bc), _dot(s_ca, s_ca)
    deg = np.where((q1 < q0)[..., None], s_bc, s_ab)
    deg = np.where((q2 < np.minimum(q0, q1))[..., None], s_ca, deg)
    conds = [~(nn > 0), (d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), den > 0]
    picks = [deg, a, b, s_ab, c, s_ca, s_bc, inner]
    shape = np.broadcast(nn, d1).shape
    region = np.zeros(shape, np.int8)
    cp = np.broadcast_to(deg, shape + (3,)).copy()
    taken = np.zeros(shape, bool)
    for k, (cond, pick) in enumerate(zip(conds, picks)):
        use = cond & ~taken
        cp[use] = np.broadcast_to(pick, shape + (3,))[use]
        region[use] = k
        taken |= cond
    assert cp.dtype == dtype
    return cp, np.sqrt(_dot(cp, cp)), region


def valid_faces(vertices, faces):
    f = np.asarray(faces, np.int64)
    ok = ((f >= 0) & (f < len(vertices))).all(axis=1)
    ok[ok] &= np.isfinite(np.asarray(vertices, np.float64)[f[ok]]).all(axis=(1, 2))
    return ok


def all_distances(points, vertices, faces, dtype=np.float64, chunk=1 << 20):
    """[n_points, n_faces] distances; +inf in the columns of invalid faces"""
    pts, v, f = np.asarray(points, np.float32), np.asarray(vertices, np.float32), np.asarray(faces, np.int64)
    ok = valid_faces(v, f)
    out = np.full((len(pts), len(f)), np.inf, dtype)
    fv = f[ok]
    rows = max(1, chunk // max(1, len(fv)))
    for i in range(0, len(pts), rows):
        p = pts[i:i + rows, None, :]
        out[i:i + rows, ok] = closest_on_triangle(p, v[fv[:, 0]][None], v[fv[:, 1]][None], v[fv[:, 2]][None], dtype)[1]
    return out


def nearest(points, vertices, faces, dtype=np.float64, max_dist=np.inf):
    """(dist [n], face [n]): the minimum over the valid faces and the LOWEST index that attains it bit for bit; max_dist's rule"""
    d = all_distances(points, vertices, faces, dtype)
    if d.shape[1] == 0:
        return np.full(len(d), np.inf, dtype), np.full(len(d), -1, np.int64)
    dist, face = d.min(axis=1), d.argmin(axis=1)             # (argmin: the first of the smallest)
    none = ~np.isfinite(dist) | (dist > max_dist)
    return np.where(none, np.inf, dist).astype(dtype), np.where(none, -1, face)


def bound_for(points, vertices, faces):
    """(bound, float32-vs-float64 error, dist64, face64, d64 matrix) of a case"""
    d64 = all_distances(points, vertices, faces, np.float64)
    d32 = all_distances(points, vertices, faces, np.float32)
    m64, m32 = d64.min(axis=1), d32.min(axis=1).astype(np.float64)
    fin = np.isfinite(m64)
    err = float(np.abs(m32[fin] - m64[fin]).max()) if fin.any() else 0.0
    scale = max(1.0, float(np.abs(np.asarray(points, np.float32)).max(initial=0)),
                float(np.abs(np.asarray(vertices, np.float32)[np.isfinite(vertices).all(axis=1)]).max(initial=0)))
    return max(4.0 * err, 2.0 ** -22 * scale), err, m64, d64.argmin(axis=1), d64


# ---------------------------------------------------------------- meshes

def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def one_triangle():
    return f32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]], np.int32)


def two_triangles():
    """two triangles sharing the edge (1,0,0)-(0,1,0), not coplanar"""
    return f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]]), np.array([[0, 1, 2], [2, 1, 3]], np.int32)


def region_queries(vertices, faces, count, seed=0):
    """`count` queries around the triangles: the first ones are constructed -- per triangle the seven regions at heights +h, -h and 0
    (in the plane), and points exactly on a vertex, an edge midpoint and the centroid-ish interior point (dyadic weights) -- the rest
    are those again, jittered"""
    v = np.asarray(vertices, np.float64)
    base = []
    for tri in np.asarray(faces):
        a, b, c = v[tri]
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        cen = (a + b + c) / 3
        inplane = [0.5 * a + 0.25 * b + 0.25 * c]                                       # interior
        for p, q, r in ((a, b, c), (b, c, a), (c, a, b)):
            mid = 0.5 * (p + q)
            out = mid - r
            out -= np.dot(out, q - p) / np.dot(q - p, q - p) * (q - p)
            inplane.append(mid + 0.25 * out / np.linalg.norm(out))                      # beside the edge pq
            inplane.append(p + 0.5 * (p - cen))                                         # beyond the vertex p
        for h in (0.375, -0.375, 0.0):
            base += [x + h * n for x in inplane]
        base += [a, b, c, 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a), 0.5 * a + 0.25 * b + 0.25 * c]     # distance exactly 0
    base = np.array(base)
    rng = np.random.default_rng(seed)
    reps = -(-count // len(base))
    pts = np.concatenate([base] + [base + rng.normal(0, 0.15, base.shape) for _ in range(reps - 1)]) if reps > 1 else base
    if count < len(base):                                    # a short list keeps a spread of the constructed points
        pts = base[np.linspace(0, len(base) - 1, count).astype(int)]
    return f32(pts[:count])


def icosahedron():
    t = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
                  [-t, 0, -1], [-t, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    return f32(v / np.linalg.norm(v[0])), f


@functools.lru_cache(maxsize=None)
def icosphere(level):
    """unit icosphere: 20 * 4^level faces (level 2: 320, level 3: 1280)"""
    v, f = icosahedron()
    v = [tuple(x) for x in v.astype(np.float64)]
    for _ in range(level):
        cache, nf = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                m = (np.array(v[i]) + np.array(v[j])) / 2
                v.append(tuple(m / np.linalg.norm(m)))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = np.array(nf, np.int32)
    return f32(v), np.ascontiguousarray(f, np.int32)


def sphere_points(n, radius, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    return f32(radius * p / np.linalg.norm(p, axis=1, keepdims=True))


def degenerate_mix():
    """the icosahedron's 20 faces, then: collinear vertices (21st face, index 20), three equal vertices (21), face 3 once more (22).
    The degenerate faces stick out of the solid so that queries near them find them."""
    v, f = icosahedron()
    extra = f32([[1.5, 0, 0], [2.0, 0, 0], [2.5, 0, 0], [0, 2.0, 0.25]])               # 12, 13, 14 collinear; 15 a lone point
    v = np.concatenate([v, extra])
    f = np.concatenate([f, [[12, 14, 13], [15, 15, 15], f[3]]]).astype(np.int32)
    return v, f


def degenerate_queries():
    """near the segment (beside it, beyond both ends), near the lone point, near face 3 / its duplicate, and a few around"""
    v, f = degenerate_mix()
    c3 = v[f[3]].astype(np.float64).mean(axis=0)
    pts = [[2.0, 0.25, 0.0], [1.75, -0.125, 0.125], [3.0, 0.0, 0.0], [2.75, 0.25, 0], [2.25, 0, 0], [0, 2.0, 0.5], [0.125, 2.25, 0.25],
           [0, 2.0, 0.25], c3 * 1.25, c3 * 1.5, c3 * 0.75]
    return f32(np.concatenate([np.array(pts), sphere_points(40, 1.75, seed=3).astype(np.float64)]))


def tie_cube():
    """a cube [-1, 1]^3 of 12 faces whose +y face is the x <-> y mirror image of its +x face, vertex for vertex, so that a point on the
    plane x = y has, operation for operation, the same float32 distance to both (the dot product adds x and y terms first)"""
    quad_x = np.array([[1, -1, -1], [1, 1, -1], [1, 1, 1], [1, -1, 1]], np.float64)                 # the +x face, corners in a cycle
    swap = lambda q, i, j: q[:, [j if k == i else i if k == j else k for k in range(3)]]
    quads = [quad_x, -quad_x, swap(quad_x, 0, 2), -swap(quad_x, 0, 2), -swap(quad_x, 0, 1), swap(quad_x, 0, 1)]     # +x -x +z -z -y +y
    v = np.concatenate(quads)
    f = np.concatenate([[[4 * k, 4 * k + 1, 4 * k + 2], [4 * k, 4 * k + 2, 4 * k + 3]] for k in range(6)]).astype(np.int32)
    return f32(v), f


def tie_queries():
    """on the plane x = y, inside the cube and nearer to +x / +y than to anything else; every coordinate a dyadic rational"""
    return f32([[1 - t, 1 - t, z] for t in (0.25, 0.125, 0.375, 0.0625) for z in (0.0, 0.125, -0.25, 0.5, -0.5625)])


def plane_mesh(nx=9, ny=7, seed=5):
    """a triangulated, jittered sheet in the plane z = 0: zero extent on one axis"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64), indexing="ij")
    v = np.stack([x + rng.uniform(-0.3, 0.3, x.shape), y + rng.uniform(-0.3, 0.3, y.shape), np.zeros_like(x)], axis=-1).reshape(-1, 3) * 0.1
    idx = lambda i, j: i * (ny + 1) + j
    f = [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(nx) for j in range(ny)]
    f += [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(nx) for j in range(ny)]
    return f32(v), np.array(f, np.int32)


def stress_mesh(n_small=2000, seed=6):
    """one long thin triangle across the whole box, then n_small tiny ones: the long one lands in a large share of the cells"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.05, 0.95, (n_small, 3))
    tri = centres[:, None, :] + rng.uniform(-0.004, 0.004, (n_small, 3, 3))
    v = np.concatenate([[[0, 0, 0], [1, 1, 1], [1, 0.98, 1]], tri.reshape(-1, 3)])
    f = np.concatenate([[[0, 1, 2]], 3 + np.arange(3 * n_small).reshape(-1, 3)])
    return f32(v), np.ascontiguousarray(f, np.int32)


def box_queries(vertices, n, seed=7, margin=0.2):
    """n points in and a little around the mesh's box"""
    v = np.asarray(vertices, np.float64)
    v = v[np.isfinite(v).all(axis=1)]
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 0.1 * (hi - lo).max())
    return f32(np.random.default_rng(seed).uniform(lo - margin * ext, hi + margin * ext, (n, 3)))


def far_queries(vertices, factor=10.0):
    """26 points at `factor` x the box's extent from its centre, in every direction of the 3 x 3 x 3 neighbourhood"""
    v = np.asarray(vertices, np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    cen, ext = 0.5 * (lo + hi), np.maximum(hi - lo, 0.1 * (hi - lo).max())
    dirs = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], np.float64)
    return f32(cen + factor * ext * dirs)


def cube_mesh(half=1.0, centre=(0, 0, 0)):
    v, f = tie_cube()
    return f32(v.astype(np.float64) * half + np.asarray(centre, np.float64)), f


# ---------------------------------------------------------------- sampling

def fmix32(h):
    """MurmurHash3's 32-bit finalizer (Appleby), on uint32 arrays"""
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85ebca6b)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xc2b2ae35)
    h ^= h >> np.uint32(16)
    return h


def sample_randoms(seed, i):
    """(r1, r2) float32 in [0, 1) of samples i (the header's counter-based rule)"""
    i = np.asarray(i, dtype=np.uint32)
    with np.errstate(over="ignore"):
        u1 = fmix32(np.uint32(seed) ^ fmix32(np.uint32(2) * i))
        u2 = fmix32(np.uint32(seed) ^ fmix32(np.uint32(2) * i + np.uint32(1)))
    scale = np.float32(2.0 ** -24)
    return (u1 >> np.uint32(8)).astype(np.float32) * scale, (u2 >> np.uint32(8)).astype(np.float32) * scale


def face_areas(vertices, faces):
    """float64 areas from the float32 vertices; 0 for an invalid face (an index out of range, a non-finite vertex)"""
    v, f = np.asarray(vertices, np.float32).astype(np.float64), np.asarray(faces, np.int64)
    ok = valid_faces(v, f)
    a, b, c = (v[f[ok, k]] for k in range(3))
    out = np.zeros(len(f))
    out[ok] = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    return out


def sample_points_np(vertices, faces, face_of, seed, dtype):
    """the points of samples 0 .. len(face_of) - 1 on the faces named for them, the header's formula in `dtype` on the same float32
    inputs (vertices and the two float32 randoms): float32 is what the kernel computes, float64 lies in the face's plane"""
    v = np.asarray(vertices, np.float32).astype(dtype)
    f = np.asarray(faces)[np.asarray(face_of)]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    r1, r2 = (r.astype(dtype) for r in sample_randoms(seed, np.arange(len(f))))
    s = np.sqrt(r1)
    wa, wb, wc = 1 - s, s * (1 - r2), s * r2
    out = (wa[:, None] * a + wb[:, None] * b) + wc[:, None] * c
    assert out.dtype == dtype
    return out


def sampling_bound(vertices, faces, face_of, seed):
    """(bound, float32-vs-float64 error) of a set of samples by the distance rule: 4 x the largest distance between the float32 and
    the float64 point of the same sample, at least floor_bound"""
    d = sample_points_np(vertices, faces, face_of, seed, np.float32).astype(np.float64) - sample_points_np(vertices, faces, face_of, seed, np.float64)
    err = float(np.sqrt((d * d).sum(axis=1)).max())
    return max(4 * err, floor_bound(np.asarray(vertices)[np.isfinite(vertices).all(axis=1)])), err


def sample_point(vertices, face, r1, r2):
    """the float32 point of a sample on `face` from its two randoms, as the header orders the operations"""
    v = np.asarray(vertices, np.float32)
    a, b, c = (v[face[k]] for k in range(3))
    s = np.sqrt(np.float32(r1))
    wa, wb, wc = np.float32(1) - s, s * (np.float32(1) - np.float32(r2)), s * np.float32(r2)
    return (wa * a + wb * b) + wc * c


def barycentrics(points, vertices, faces, face_of):
    """float64 (u, v, w) of each point in its face's plane and its distance to that plane"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    tri = v[np.asarray(faces)[face_of]]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    p = np.asarray(points, np.float32).astype(np.float64)
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(axis=1)
    w_a = (np.cross(b - p, c - p) * n).sum(axis=1) / nn
    w_b = (np.cross(c - p, a - p) * n).sum(axis=1) / nn
    w_c = (np.cross(a - p, b - p) * n).sum(axis=1) / nn
    return np.stack([w_a, w_b, w_c], axis=1), np.abs(((p - a) * n).sum(axis=1)) / np.sqrt(nn)


# ---------------------------------------------------------------- stats

def stats_values(n, seed=9):
    """float32 values with NaN, +inf and finite mixed"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0, 0.05, n).astype(np.float32)
    kind = rng.integers(0, 10, n)
    v[kind == 0] = np.nan
    v[kind == 1] = np.inf
    v[(kind == 2) & (np.arange(n) % 7 == 0)] = -np.inf       # (no distance is; the entry point takes any list)
    return v


def stats_np(values, thresholds):
    """gpnerf_distance_stats' slot restated: (finite, inf, nan counts, mean, mean of squares, max, [within counts], non-NaN count)"""
    v = np.asarray(values, np.float32)
    nan, inf = np.isnan(v), np.isinf(v)
    fin = v[~nan & ~inf].astype(np.float64)
    mean, sq, mx = (float(fin.mean()), float((fin * fin).mean()), float(fin.max())) if len(fin) else (np.nan, np.nan, np.nan)
    within = [int((v[~nan & ~inf] <= np.float32(t)).sum()) for t in thresholds]      # an infinite value of either sign is not within
    return len(fin), int(inf.sum()), int(nan.sum()), mean, sq, mx, within, int((~nan).sum())


# ---------------------------------------------------------------- a body-sized mesh

def nearest_pruned(points, vertices, faces):
    """(dist64 [n], dist32 [n]) like `nearest`, for a mesh too large to test every face in numpy within a test's seconds: per query
    the faces are first cut down by their bounding boxes -- a face whose box is farther than the nearest box's farthest corner
    (with a 0.1 % margin) cannot hold the minimum -- and THE DISTANCE runs on the rest.  Still the exact minimum over all faces."""
    pts, v, f = np.asarray(points, np.float32), np.asarray(vertices, np.float32).astype(np.float64), np.asarray(faces, np.int64)
    assert valid_faces(v, f).all()
    tri = v[f]
    lo, hi = tri.min(axis=1), tri.max(axis=1)
    d64, d32 = np.empty(len(pts)), np.empty(len(pts))
    for i, p in enumerate(pts.astype(np.float64)):
        near = np.sqrt((np.maximum(np.maximum(lo - p, p - hi), 0) ** 2).sum(axis=1))
        far = np.sqrt((np.maximum(np.abs(p - lo), np.abs(p - hi)) ** 2).sum(axis=1))
        keep = near <= far.min() * 1.001
        a, b, c = (v[f[keep, k]] for k in range(3))
        d64[i] = closest_on_triangle(pts[i], a, b, c, np.float64)[1].min()
        d32[i] = closest_on_triangle(pts[i], a, b, c, np.float32)[1].min()
    return d64, d32


def distance_to_face(points, vertices, faces, face_of):
    """float64 distance of each point to the one face named for it"""
    v, f = np.asarray(vertices, np.float32), np.asarray(faces, np.int64)[np.asarray(face_of)]
    return closest_on_triangle(np.asarray(points, np.float32), v[f[:, 0]], v[f[:, 1]], v[f[:, 2]], np.float64)[1]


def floor_bound(*arrays):
    """2^-22 max(1, max |coordinate|): the least a distance bound can be"""
    m = max(float(np.abs(a[np.isfinite(a)]).max(initial=0)) for a in (np.asarray(x, np.float64) for x in arrays))
    return 2.0 ** -22 * max(1.0, m)
