"""A numpy / scipy restatement of gpnerf_cube_clean and gpnerf_mesh_normals (the specification in include/gpnerf_hip.h), the cubes the
tests run them on, and the surface-counting helper."""
import numpy as np
from scipy import ndimage

import mesh_cases as mc

S18 = ndimage.generate_binary_structure(3, 2)         # 6 face + 12 face-diagonal neighbours: the solid
S6 = ndimage.generate_binary_structure(3, 1)          # 6 face neighbours: the outside
KEEP, FILL = 1, 2
STATS = ("components", "inside_points", "components_kept", "inside_points_kept", "cavities_filled", "points_filled")
MODES = {"largest": (KEEP, 0), "min64": (KEEP, 64), "fill": (FILL, 0), "both": (KEEP | FILL, 0)}


def components(mask, structure):
    """(labels int32 like mask: the lowest linear index of each set point's component, -1 elsewhere; sizes by that label, a dict)."""
    lab, n = ndimage.label(mask, structure=structure)
    flat = lab.reshape(-1)
    out = -np.ones(flat.shape, dtype=np.int32)
    sizes = {}
    if n:
        idx = np.nonzero(flat)[0]
        first = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat[idx], idx)           # the lowest linear index of every component
        out[idx] = first[flat[idx]].astype(np.int32)
        count = np.bincount(flat, minlength=n + 1)
        sizes = {int(first[k]): int(count[k]) for k in range(1, n + 1)}
    return out.reshape(mask.shape), sizes


def clean_np(cube, iso, flags=0, min_points=0):
    """(out_cube float32, labels int32, stats int64[6]) by the header's rules."""
    f = np.ascontiguousarray(cube, dtype=np.float32)
    iso = np.float32(iso)
    inside = ~(f < iso)
    labels, sizes = components(inside, S18)
    stats = np.zeros(6, dtype=np.int64)
    stats[0], stats[1] = len(sizes), int(inside.sum())
    out = f.copy()
    kept = set(sizes)
    if flags & KEEP:
        if min_points > 0:
            kept = {k for k, n in sizes.items() if n >= min_points}
        elif sizes:
            top = max(sizes.values())
            kept = {min(k for k, n in sizes.items() if n == top)}        # a tie goes to the lower label
    stats[2], stats[3] = len(kept), sum(sizes[k] for k in kept)
    if len(kept) != len(sizes):
        drop = inside & ~np.isin(labels, np.fromiter(kept, dtype=np.int32, count=len(kept)))
        out[drop] = np.float32(0.0)
    if flags & FILL:
        below = out < iso
        lab, n = ndimage.label(below, structure=S6)
        if n:
            open_ = np.zeros(n + 1, dtype=bool)                        # components that reach one of the six boundary faces
            for ax in range(3):
                for side in (0, -1):
                    open_[np.unique(np.take(lab, side, axis=ax))] = True
            open_[0] = True
            cavity = ~open_[lab]
            stats[4], stats[5] = int((~open_).sum()), int(cavity.sum())
            out[cavity] = np.float32(1.0)
    return out, labels, stats


def surfaces(faces, n_vertices):
    """number of connected surfaces of a triangle list (vertices joined by the triangles' edges)"""
    if len(faces) == 0:
        return 0
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    i = np.concatenate([faces[:, 0], faces[:, 1]])
    j = np.concatenate([faces[:, 1], faces[:, 2]])
    g = coo_matrix((np.ones(len(i), dtype=np.int8), (i, j)), shape=(n_vertices, n_vertices))
    _, lab = connected_components(g, directed=False)
    return len(np.unique(lab[np.unique(faces)]))


def triangle_set(verts, faces):
    """the triangles as a sorted array of their nine position words (uint32 views): equal positions <=> equal rows"""
    t = np.ascontiguousarray(verts, dtype=np.float32).view(np.uint32)[faces].reshape(len(faces), 9)
    return np.unique(t, axis=0)


def is_subset(tri_a, tri_b):
    """every row of tri_a (triangle_set) is a row of tri_b"""
    both = np.unique(np.concatenate([tri_a, tri_b]), axis=0)
    return len(both) == len(tri_b)


def normals_np(cube, verts, inv_step=None, dtype=np.float32):
    """(normals, |g|) by the header's formula, every operation in `dtype` (float32: the device's arithmetic; float64: the yardstick)."""
    T = dtype
    f = np.ascontiguousarray(cube, dtype=np.float32).astype(T)
    v = np.ascontiguousarray(verts, dtype=np.float32).astype(T)
    inv = np.ones(3, dtype=T) if inv_step is None else np.asarray(inv_step, dtype=np.float32).astype(T)
    dims = np.array(f.shape)
    i = np.clip(np.floor(v), 0, dims - 2).astype(np.int64)
    t = (v - i.astype(T)).astype(T)
    half = T(0.5)

    def G(p, a):
        hi, lo = p.copy(), p.copy()
        hi[:, a] = np.minimum(hi[:, a] + 1, dims[a] - 1)
        lo[:, a] = np.maximum(lo[:, a] - 1, 0)
        return ((f[hi[:, 0], hi[:, 1], hi[:, 2]] - f[lo[:, 0], lo[:, 1], lo[:, 2]]) * half) * inv[a]

    lerp = lambda a, b, w: a + w * (b - a)
    g = np.zeros(v.shape, dtype=T)
    for a in range(3):
        c = {}
        for k in range(8):
            d = np.array([k >> 2, (k >> 1) & 1, k & 1])
            c[k] = G(i + d, a)
        z = [lerp(c[0], c[1], t[:, 2]), lerp(c[2], c[3], t[:, 2]), lerp(c[4], c[5], t[:, 2]), lerp(c[6], c[7], t[:, 2])]
        g[:, a] = lerp(lerp(z[0], z[1], t[:, 1]), lerp(z[2], z[3], t[:, 1]), t[:, 0])
    with np.errstate(all="ignore"):
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = (length > 0) & np.isfinite(length)
        n = np.where(ok[:, None], -g / np.where(ok, length, T(1))[:, None], T(0))
    return n.astype(T), length


# ---- the cubes ---------------------------------------------------------------------------------------------------------------------
NOISE_TIE_ISO = 0.0385      # noise_cube() at this iso: thousands of small solid components, several tied for the largest


def noise_cube():
    """Odd sizes, bricks cut by the cube's end.  At iso 0.02 the solid percolates (a handful of components) and the outside breaks
    into hundreds of cavities; at NOISE_TIE_ISO the solid is thousands of components with many size ties, the largest included."""
    return np.pad(np.random.default_rng(5).uniform(0, 0.04, (37, 61, 45)).astype(np.float32), 1)


def snakes_cube(dims=(40, 40, 72)):
    """Two one-voxel-wide snakes of equal length: snake A runs along z on the rows (x, y) with x % 4 == 0, y % 4 == 0, joined at
    alternating z ends (a boustrophedon over y, then over x); snake B is A shifted by (2, 2, 0).  They are two voxels apart
    everywhere (not 18-connected), each passes through every 4 x 8 x 32 brick several times, and both have the same number of points."""
    c = np.zeros(dims, dtype=np.float32)
    nx, ny, nz = dims
    for off in (0, 2):
        xs, ys = list(range(off, nx - 1, 4)), list(range(off, ny - 1, 4))
        rows = [(x, y) for i, x in enumerate(xs) for y in (ys if i % 2 == 0 else ys[::-1])]
        for k, (x, y) in enumerate(rows):
            c[x, y, 1:nz - 1] = 1
            if k + 1 < len(rows):                       # the bridge to the next row, at alternating z ends
                x2, y2 = rows[k + 1]
                zend = nz - 2 if k % 2 == 0 else 1
                c[min(x, x2):max(x, x2) + 1, min(y, y2):max(y, y2) + 1, zend] = 1
    return c


def diagonal_pairs_cube():
    """Pairs of points that touch only across a face diagonal (one component) or only across a body diagonal (two), every pair placed
    to straddle a brick boundary (bricks are 4 x 8 x 32) along x, y and z.  Returns (cube, expected number of components)."""
    c = np.zeros((12, 20, 70), dtype=np.float32)
    n = 0
    face = [((1, 1, 0), (3, 7, 10)), ((1, 0, 1), (3, 3, 31)), ((0, 1, 1), (1, 7, 31)), ((1, -1, 0), (3, 8, 20)), ((1, 0, -1), (3, 12, 32)),
            ((0, 1, -1), (9, 7, 32)), ((1, 1, 0), (7, 15, 40)), ((0, 1, 1), (6, 15, 63))]
    for d, p in face:
        c[p] = 1
        c[tuple(np.add(p, d))] = 1
        n += 1
    body = [((1, 1, 1), (3, 7, 50)), ((1, -1, 1), (3, 8, 31)), ((1, 1, -1), (3, 15, 64)), ((1, -1, -1), (7, 16, 32))]
    for d, p in body:
        c[p] = 1
        c[tuple(np.add(p, d))] = 1
        n += 2
    return c, n


def shell_cube(tunnel=False, diagonal_leak=False):
    """A solid box (walls 2 to 3 voxels thick) with a hollow that crosses brick boundaries in x, y and z.  tunnel: a one-voxel tunnel
    from the hollow to the z = 0 face, which makes the hollow exterior.  diagonal_leak: instead, a slit through the x wall whose three
    voxels touch one another only across face diagonals -- the first joins the hollow, the last the exterior, the middle one is a
    one-point cavity of its own: under 6-connectivity nothing leaks, both cavities are filled."""
    c = np.zeros((14, 22, 76), dtype=np.float32)
    c[1:13, 2:20, 3:72] = 1
    c[3:10, 5:17, 20:60] = 0            # the hollow: x 3..9, y 5..16, z 20..59 (crosses x = 4, 8; y = 8, 16; z = 32)
    if tunnel:
        c[6, 10, 0:20] = 0
    if diagonal_leak:
        c[10, 10, 30] = 0               # a face neighbour of the hollow's (9, 10, 30)
        c[11, 11, 30] = 0               # a face-diagonal step
        c[12, 12, 30] = 0               # another; (13, 12, 30) beyond it is exterior
    return c


def floater_bubble_cube():
    """a big solid block, and a smaller hollow floater beside it: KEEP "largest" removes the floater, which opens its bubble"""
    c = np.zeros((16, 24, 70), dtype=np.float32)
    c[1:15, 1:12, 1:69] = 1             # the body
    c[2:12, 14:23, 5:45] = 1            # the floater ...
    c[4:10, 16:21, 10:40] = 0           # ... and its bubble
    return c


def faces_touching_cube():
    """components that touch the cube's faces, and a below-iso pocket open only through a face"""
    c = np.zeros((9, 17, 40), dtype=np.float32)
    c[0:3, 0:5, 0:6] = 1                # a corner block on three faces
    c[6:9, 10:17, 30:40] = 1            # the opposite corner
    c[3:6, 6:10, 0:12] = 1              # on the z = 0 face, with a pocket open to that face only
    c[4, 7:9, 0:8] = 0
    c[4, 12, 20] = 1                    # an interior single point
    return c


def small_cubes():
    one = np.ones((5, 9, 33), dtype=np.float32)
    r = np.random.default_rng(9)
    return {"d222": (r.uniform(0, 0.04, (2, 2, 2)).astype(np.float32)), "d35130": r.uniform(0, 0.04, (3, 5, 130)).astype(np.float32),
            "all_inside": one, "all_outside": 0 * one}
