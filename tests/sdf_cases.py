"""The truncated signed distance field (gpnerf_sdf.hip) restated in numpy from the text of include/gpnerf_hip.h, the trilinear
sampling restated in float64, and the cases of their tests.  Nothing here looks at what the kernels give.

The distance is tests/mesh_metric_cases.py's `closest_on_triangle`, THE DISTANCE of the header operation for operation: run in float32
it is what the kernels compute, run in float64 it is the reference of DESIGN 4.10's bound.  The restatement follows the DEFINITION, not
the kernels' boxes: the minimum runs over every USED face.  To stay within a test's seconds it leaves out (face, point) pairs that
cannot matter by a bound of its own -- a point farther than 1.01 band + 1e-3 from the face's bounding SPHERE has a true distance above
that and a computed one above the band (the distance function errs by 2^-20 of distance + diameter) -- which is not the kernels' rule
(an axis-aligned box widened by one step), so the PAIRS count and the minima check that rule rather than repeat it."""
import functools

import numpy as np

import mesh_metric_cases as mm
import voxelize_cases as vc

GUARD = 2.0 ** 16
LARGE_POINTS = 64                                            # box points above which the kernels give a face a wavefront
MAX_BAND_STEPS = 1024
STATS = ("used", "skipped_vertex", "skipped_box", "large", "in_band", "inside", "visited", "pairs")


# ---------------------------------------------------------------- the definition

def lattice_points(lo, step, dims):
    """float32 [nx,ny,nz,3]: P_a = float32(lo_a + i_a * step_a), product and sum in float64"""
    lo, step = np.asarray(lo, np.float64).reshape(3), np.asarray(step, np.float64).reshape(3)
    ax = [(lo[a] + np.arange(dims[a], dtype=np.float64) * step[a]).astype(np.float32) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def face_states(vertices, faces, lo, step):
    """(indices int64 [m,3] with bad ones replaced by 0, skipped-for-a-vertex bool [m]): an index out of range, or a vertex with a u
    that is not finite or beyond 2^16 steps on any axis"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < len(v))).all(axis=1)
    fs = np.where(in_range[:, None], f, 0)
    if not len(v):
        return fs, np.ones(len(f), bool)
    with np.errstate(all="ignore"):
        u = (v - np.asarray(lo, np.float64)[None]) / np.asarray(step, np.float64)[None]
        usable = (np.abs(u) <= GUARD).all(axis=1)            # (false for a NaN)
    return fs, ~in_range | ~usable[fs].all(axis=1)


def face_boxes(vertices, tri, lo, step, dims, band):
    """(i0 int64 [m,3], i1 int64 [m,3]) of usable faces `tri` [m,3]: the header's float64 expressions, clipped; empty where i1 < i0"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    lo, step = np.asarray(lo, np.float64).reshape(3), np.asarray(step, np.float64).reshape(3)
    band = np.float64(np.float32(band))
    corners = v[tri]                                         # float32 [m,3,3]
    mn, mx = corners.min(axis=1).astype(np.float64), corners.max(axis=1).astype(np.float64)
    i0 = np.ceil(((mn - band) - lo[None]) / step[None]) - 1.0
    i1 = np.floor(((mx + band) - lo[None]) / step[None]) + 1.0
    top = np.asarray(dims, np.float64)[None] - 1.0
    return np.maximum(i0, 0.0).astype(np.int64), np.minimum(i1, top).astype(np.int64)


def _candidate_pairs(points64, vertices, tri, band, chunk=1 << 22):
    """(point index, face row) pairs that can matter: the point lies within 1.01 band + 1e-3 of the face's bounding sphere"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    corners = v[tri]
    centre = corners.mean(axis=1)
    radius = np.sqrt(((corners - centre[:, None]) ** 2).sum(axis=2)).max(axis=1)
    reach = radius + 1.01 * float(band) + 1e-3
    pi, fi = [], []
    rows = max(1, chunk // max(1, len(tri)))
    for s in range(0, len(points64), rows):
        d = points64[s:s + rows, None, :] - centre[None]
        near = (d * d).sum(axis=2) <= (reach * reach)[None]
        a, b = np.nonzero(near)
        pi.append(a + s)
        fi.append(b)
    return np.concatenate(pi), np.concatenate(fi)


def sdf_np(vertices, faces, lo, step, dims, band, occ=None, want64=True):
    """-> dict(abs float32 [nx,ny,nz]: min(m, band); face int64: the lowest face at the minimum's bits, -1 beyond the band; sdf float32:
    abs with the sign of `occ` (bool cube or None); stats int64 [8]; tie bool: more than one face at the minimum's bits, in band;
    boxes int64 [used]: box sizes of the used faces (0: skipped for its box); abs64 float64: the same minimum in float64, truncated;
    err: the largest float32-vs-float64 difference of a pair's distance over the candidate pairs; edge: the least |m64 - band| over the
    points, how far the case is from a point whose IN_BAND could flip)"""
    dims = tuple(int(d) for d in dims)
    band32 = np.float32(band)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    fs, bad = face_states(v, faces, lo, step)
    ok = np.nonzero(~bad)[0]
    tri = fs[ok]
    i0, i1 = face_boxes(v, tri, lo, step, dims, band32) if len(ok) else (np.zeros((0, 3), np.int64),) * 2
    widths = np.maximum(i1 - i0 + 1, 0)
    boxes = np.where((widths > 0).all(axis=1), widths.prod(axis=1), 0)
    used = boxes > 0
    P = lattice_points(lo, step, dims).reshape(-1, 3)
    n = len(P)
    m32, m64 = np.full(n, np.inf, np.float32), np.full(n, np.inf)
    face = np.full(n, -1, np.int64)
    ties = np.zeros(n, np.int64)
    pairs, err = 0, 0.0
    if used.any():
        ut = tri[used]
        pi, fr = _candidate_pairs(P.astype(np.float64), v, ut, band32)
        a, b, c = v[ut[fr, 0]], v[ut[fr, 1]], v[ut[fr, 2]]
        d32 = mm.closest_on_triangle(P[pi], a, b, c, np.float32)[1]
        assert d32.dtype == np.float32
        np.minimum.at(m32, pi, d32)
        at = d32 == m32[pi]
        fidx = ok[used][fr]
        lowest = np.full(n, np.iinfo(np.int64).max)
        np.minimum.at(lowest, pi[at], fidx[at])
        np.add.at(ties, pi[at], 1)
        face = np.where(np.isfinite(m32), lowest, -1)
        pairs = int((d32 <= band32).sum())
        if want64:
            d64 = mm.closest_on_triangle(P[pi], a, b, c, np.float64)[1]
            np.minimum.at(m64, pi, d64)
            err = float(np.abs(d32.astype(np.float64) - d64).max()) if len(d64) else 0.0
    hit = m32 <= band32
    absv = np.where(hit, m32, band32).astype(np.float32)
    face = np.where(hit, face, -1)
    inside = np.zeros(n, bool) if occ is None else np.asarray(occ, bool).reshape(-1)
    sdf = np.where(inside, -absv, absv).astype(np.float32)
    stats = np.array([int(used.sum()), int(bad.sum()), int((~used).sum()), int((boxes > LARGE_POINTS).sum()), int(hit.sum()), int(inside.sum()),
                      int(boxes.sum()), pairs], np.int64)
    edge = float(np.abs(m64[np.isfinite(m64)] - float(band32)).min()) if want64 and np.isfinite(m64).any() else np.inf
    return dict(abs=absv.reshape(dims), face=face.reshape(dims), sdf=sdf.reshape(dims), stats=stats, tie=(hit & (ties > 1)).reshape(dims),
                boxes=boxes, abs64=np.minimum(m64, float(band32)).reshape(dims), err=err, edge=edge)


def nearest64(points, vertices, faces, reach):
    """float64 [n]: the distance of float64 points (rounded to float32, as THE DISTANCE takes them) to a mesh of valid faces, exact
    wherever it is under `reach` and inf elsewhere"""
    p = mm.f32(points)
    tri = np.asarray(faces, np.int64)
    v = np.asarray(vertices, np.float32)
    pi, fr = _candidate_pairs(p.astype(np.float64), v, tri, reach)
    d = mm.closest_on_triangle(p[pi], v[tri[fr, 0]], v[tri[fr, 1]], v[tri[fr, 2]], np.float64)[1]
    out = np.full(len(p), np.inf)
    np.minimum.at(out, pi, d)
    return out


def bound_of(ref, vertices, faces, lo, step, dims):
    """DESIGN 4.10's bound for a case: 4 x the float32-vs-float64 difference of the restatement, at least 2^-22 max(1, max |coordinate|)
    over the lattice and the vertices of the faces that are not skipped for a vertex (no other coordinate enters the arithmetic)"""
    fs, bad = face_states(vertices, faces, lo, step)
    v = np.asarray(vertices, np.float64).reshape(-1, 3)[np.unique(fs[~bad])] if (~bad).any() else np.zeros((0, 3))
    hi = np.asarray(lo, np.float64) + (np.asarray(dims, np.float64) - 1) * np.asarray(step, np.float64)
    return max(4.0 * ref["err"], mm.floor_bound(v, np.asarray(lo, np.float64), hi))


def sample_np(values, lo, step, points):
    """gpnerf_sdf_sample restated in float64 -> float32 [n]: z, then y, then x, each as a + t (b - a); one rounding"""
    f = np.asarray(values, np.float32).astype(np.float64)
    dims = np.array(f.shape, np.float64)
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        u = (p - np.asarray(lo, np.float64)[None]) / np.asarray(step, np.float64)[None]
        ok = ((u >= 0.0) & (u <= dims[None] - 1.0)).all(axis=1)          # (false for a NaN)
    us = np.where(ok[:, None], u, 0.0)
    c = np.minimum(np.floor(us), dims[None] - 2.0)
    t = us - c
    i, j, k = (c[:, a].astype(np.int64) for a in range(3))
    lerp = lambda a, b, w: a + w * (b - a)
    z = [[lerp(f[i + di, j + dj, k], f[i + di, j + dj, k + 1], t[:, 2]) for dj in (0, 1)] for di in (0, 1)]
    y = [lerp(z[di][0], z[di][1], t[:, 1]) for di in (0, 1)]
    out = lerp(y[0], y[1], t[:, 0])
    return np.where(ok, out, np.nan).astype(np.float32)


def sample_direct(values, lo, step, points):
    """the eight-corner formula, float64 [n]: sum over the corners of value x the product of the three weights (inside points only)"""
    f = np.asarray(values, np.float32).astype(np.float64)
    dims = np.array(f.shape, np.float64)
    u = (np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64) - np.asarray(lo, np.float64)[None]) / np.asarray(step, np.float64)[None]
    c = np.minimum(np.floor(u), dims[None] - 2.0)
    t = u - c
    i, j, k = (c[:, a].astype(np.int64) for a in range(3))
    out = np.zeros(len(u))
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                w = (t[:, 0] if di else 1 - t[:, 0]) * (t[:, 1] if dj else 1 - t[:, 1]) * (t[:, 2] if dk else 1 - t[:, 2])
                out += w * f[i + di, j + dj, k + dk]
    return out


def edge_crossings(values, lo, step, offset):
    """float64 [n,3]: where the surface `values = offset` crosses the lattice's edges, by marching cubes' rule on (-values, iso = -offset):
    an edge whose ends differ in (-value < -offset), the crossing at t = (iso - f0) / (f1 - f0) along it, in the lattice's frame"""
    f = -np.asarray(values, np.float32).astype(np.float64)
    iso = -float(offset)
    lo, step = np.asarray(lo, np.float64), np.asarray(step, np.float64)
    below = f < iso
    out = []
    for a in range(3):
        s0 = [slice(None)] * 3
        s1 = [slice(None)] * 3
        s0[a], s1[a] = slice(0, -1), slice(1, None)
        cross = below[tuple(s0)] != below[tuple(s1)]
        idx = np.argwhere(cross).astype(np.float64)
        f0, f1 = f[tuple(s0)][cross], f[tuple(s1)][cross]
        idx[:, a] += (iso - f0) / (f1 - f0)
        out.append(lo[None] + idx * step[None])
    return np.concatenate(out)


# ---------------------------------------------------------------- the cases

def quad_mesh(x0, y0, x1, y1, z):
    """two triangles over [x0, x1] x [y0, y1]; z: one height or four (corners in a cycle from (x0, y0))"""
    z = np.broadcast_to(np.asarray(z, np.float64), (4,))
    return mm.f32([[x0, y0, z[0]], [x1, y0, z[1]], [x1, y1, z[2]], [x0, y1, z[3]]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


NAMES = ("one_triangle", "degenerate_mix", "icosphere2", "quad_large", "both_tiers", "half_outside", "beyond_band", "invalid", "twice",
         "tie_box")
UNIT = (1.0, 1.0, 1.0)


def _case(name):
    """-> (vertices, faces, lo, step, dims, band, rule)"""
    if name == "one_triangle":
        return mm.one_triangle() + ((-0.45, -0.55, -0.5), (0.13, 0.14, 0.125), (14, 13, 9), 0.31, None)
    if name == "degenerate_mix":                              # collinear, three equal vertices, a face listed again far down the list
        return mm.degenerate_mix() + ((-1.13, -1.17, -1.11), (0.2, 0.21, 0.2), (21, 17, 12), 0.45, None)
    if name == "icosphere2":
        return mm.icosphere(2) + ((-1.33, -1.27, -1.21), (0.12, 0.12, 0.12), (23, 22, 21), 0.3, "nonzero")
    if name == "quad_large":                                  # both faces span the lattice: 40 x 40 x 7 or 8 points each, the wavefront tier
        return quad_mesh(-5.0, -5.0, 50.0, 50.0, (15.3, 16.1, 17.2, 16.6)) + ((0.0, 0.0, 0.0), UNIT, (40, 40, 33), 2.5, None)
    if name == "both_tiers":                                  # a sphere of faces 0.4 step long under a band of 0.6 step; a box of large ones
        return vc.join(vc.placed_sphere(2, 1.2, (6.3, 5.2, 7.1)), vc.box_mesh((10.5, 3.5, 2.5), (17.5, 14.5, 12.5))) + (
            (0.0, 0.0, 0.0), UNIT, (20, 18, 16), 0.6, "nonzero")
    if name == "half_outside":                                # a sphere whose centre lies a step outside the lattice's x = 0 side
        return vc.placed_sphere(1, 3.7, (-1.0, 5.2, 4.1)) + ((0.0, 0.0, 0.0), UNIT, (12, 10, 9), 1.5, "nonzero")
    if name == "beyond_band":                                 # a second sphere 18 steps off the lattice: every face of it skipped for its box
        return vc.join(vc.placed_sphere(1, 2.6, (5.3, 4.6, 4.2)), vc.placed_sphere(1, 2.6, (30.3, 4.6, 4.2))) + (
            (0.0, 0.0, 0.0), UNIT, (12, 10, 9), 1.25, "parity")
    if name == "invalid":                                     # an index == n_vertices, a negative index, a NaN vertex, an infinite vertex
        v, f = vc.placed_sphere(1, 2.6, (5.3, 4.6, 4.2))
        n = len(v)
        v = np.concatenate([v, mm.f32([[np.nan, 1.0, 1.0], [1.0, 1.0, np.inf]])])
        f = np.concatenate([[[0, 1, n + 2], [-1, 2, 3]], f, [[0, 1, n], [0, 1, n + 1]]])
        return mm.f32(v), np.ascontiguousarray(f, np.int32), (0.0, 0.0, 0.0), UNIT, (12, 10, 9), 1.25, "nonzero"
    if name == "twice":                                       # the same face twice: every distance ties, the lower index wins
        v, _ = mm.one_triangle()
        return v, np.array([[0, 1, 2], [0, 1, 2]], np.int32), (-0.45, -0.55, -0.5), (0.13, 0.14, 0.125), (14, 13, 9), 0.31, None
    if name == "tie_box":                                     # a cube on a dyadic lattice (lifted off it in z): points with x == y are as far from +x as from +y
        return mm.cube_mesh(1.0, (0.0, 0.0, 0.1)) + ((-1.5, -1.5, -1.5), (0.25, 0.25, 0.25), (13, 13, 13), 0.55, "nonzero")
    if name == "guard":                                       # a vertex 70 000 steps away on z: skipped here, though the voxeliser would take it
        v, f = vc.placed_sphere(1, 2.6, (5.3, 4.6, 4.2))
        n = len(v)
        v = np.concatenate([v, mm.f32([[2.0, 2.0, 70000.0]])])
        return mm.f32(v), np.ascontiguousarray(np.concatenate([f, [[0, 1, n]]]), np.int32), (0.0, 0.0, 0.0), UNIT, (12, 10, 9), 1.25, None
    if name == "plane":                                       # z = 0 under the whole lattice: z = +-0.5 is exactly the band away
        return quad_mesh(-4.0, -4.0, 4.0, 4.0, 0.0) + ((-1.0, -1.0, -1.0), (0.25, 0.25, 0.25), (12, 10, 9), 0.5, None)
    if name == "offset_sphere":                               # test 7: radius 1, step 0.1, band 0.5
        return mm.icosphere(2) + ((-1.43, -1.47, -1.44), (0.1, 0.1, 0.1), (30, 30, 30), 0.5, "nonzero")
    if name in ("box_nz9", "box_nz33", "box_nz64"):           # the voxeliser's word-boundary lattices
        return vc._case(name) + (1.5, "nonzero")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, want64=True):
    """-> dict(v, f, lo, step, dims, band, rule, occ, ref, bound): the mesh, the lattice, the restated occupancy under `rule` (None: no
    sign) and the restatement's result (computed once, shared, read-only)"""
    v, f, lo, step, dims, band, rule = _case(name)
    lo, step = np.array(lo, np.float64), np.array(step, np.float64)
    occ = None
    if rule is not None:
        vox = vc.voxelize_np(v, f, lo, step, dims, rule)
        vc.assert_preconditions(vox)
        occ = vox["occ"]
    ref = sdf_np(v, f, lo, step, dims, band, occ, want64)
    bound = bound_of(ref, v, f, lo, step, dims) if want64 else None
    if want64 and name != "plane":                            # no point sits where an ulp decides IN_BAND (the plane's do, exactly, on purpose)
        assert ref["edge"] > bound, (name, ref["edge"], bound)
    for a in (v, f, lo, step, ref["abs"], ref["face"], ref["sdf"], ref["stats"], ref["tie"]):
        a.setflags(write=False)
    return dict(v=v, f=f, lo=lo, step=step, dims=tuple(int(d) for d in dims), band=float(np.float32(band)), rule=rule, occ=occ, ref=ref,
                bound=bound)
