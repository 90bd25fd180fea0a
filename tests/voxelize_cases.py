"""The mesh voxeliser (gpnerf_voxelize.hip) restated in numpy from the text of include/gpnerf_hip.h -- float64 and int64, every used
face over its column box, np.add.at on the toggle rows, a suffix sum down each column -- and the cases of its tests.  Nothing here
looks at what the kernels give.

Both sides evaluate the same unfused float64 expressions on the same float32 inputs, and ownership is exact integer arithmetic, so
bits and counts are compared for EQUALITY.  The one place where another operation order could decide differently is the ceil of a
crossing's z: `case()` asserts of every case it hands out that no crossing lies within MARGIN of a lattice index -- except a column
through a vertex, which receives that vertex's Z exactly on both sides.  (The snap needs no such margin: (p - lo) / step and the
product with 4096 are single IEEE operations on both sides, so a tie is the same tie.)  The cases keep horizontal faces at
half-integer z for that reason."""
import functools

import numpy as np

import mesh_cases
import mesh_metric_cases as mm

GUARD = 2.0 ** 16
SNAP = 4096
MARGIN = 1e-9
STATS = ("used", "skipped_vertex", "skipped_area", "crossings", "open_columns", "occupied")
ISO = np.float32(0.02)


# ---------------------------------------------------------------- the definition

def lattice_units(vertices, lo, step):
    """(usable bool [n], X int64 [n], Y int64 [n], Z float64 [n], u float64 [n,3]) of float32 vertices"""
    p = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    lo, step = np.asarray(lo, np.float64).reshape(3), np.asarray(step, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        u = (p - lo[None]) / step[None]
        usable = np.isfinite(u).all(axis=1) & (np.abs(u[:, 0]) <= GUARD) & (np.abs(u[:, 1]) <= GUARD)
        X = np.where(usable, np.rint(4096.0 * np.where(usable, u[:, 0], 0.0)), 0.0).astype(np.int64)
        Y = np.where(usable, np.rint(4096.0 * np.where(usable, u[:, 1], 0.0)), 0.0).astype(np.int64)
    return usable, X, Y, u[:, 2], u


def face_states(faces, n_vertices, usable, X, Y):
    """(indices int64 [m,3] with bad ones replaced by 0, skipped-for-a-vertex bool, skipped-for-area bool, A int64) per face"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < n_vertices)).all(axis=1)
    fs = np.where(in_range[:, None], f, 0)
    if not n_vertices:
        return fs, np.ones(len(f), bool), np.zeros(len(f), bool), np.zeros(len(f), np.int64)
    bad = ~in_range | ~usable[fs].all(axis=1)
    a, b, c = fs[:, 0], fs[:, 1], fs[:, 2]
    A = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
    return fs, bad, ~bad & (A == 0), A


def _edge_in(e, s, dx, dy):
    """s E > 0, or E == 0 and (s dy < 0, or s dy == 0 and s dx > 0)"""
    return (s * e > 0) | ((e == 0) & ((s * dy < 0) | ((s * dy == 0) & (s * dx > 0))))


def pack_bits(occ):
    """bool [nx,ny,nz] -> uint32 [nx,ny,ceil(nz/32)]: point k is bit k & 31 of word k >> 5"""
    nx, ny, nz = occ.shape
    nzw = (nz + 31) // 32
    padded = np.zeros((nx, ny, nzw * 32), np.uint64)
    padded[:, :, :nz] = occ
    return (padded.reshape(nx, ny, nzw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


def unpack_bits(bits, nz):
    b = np.asarray(bits, np.uint32)
    return ((b[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(b.shape[0], b.shape[1], -1)[:, :, :nz]


def voxelize_np(vertices, faces, lo, step, dims, rule="parity"):
    """-> dict(occ bool [nx,ny,nz], bits uint32 [nx,ny,nzw], stats int64 [6], open bool [nx,ny], margin: the least distance of a
    crossing that is no vertex hit from a lattice index (inf when there is none), boxes int64 [used]: the columns in each used face's
    clipped box, kc int64: the places 0 .. nz that hold a crossing)"""
    nx, ny, nz = (int(d) for d in dims)
    usable, X, Y, Z, _ = lattice_units(vertices, lo, step)
    fs, bad, flat, A = face_states(faces, len(usable), usable, X, Y)
    used = np.nonzero(~bad & ~flat)[0]
    tri, area = fs[used], A[used]
    s = np.sign(area)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    count = np.zeros((nx, ny, nz + 1), np.int64)            # crossings at each place kc
    signed = np.zeros((nx, ny, nz + 1), np.int64)           # and the sum of their s
    n_cross, margin, boxes = 0, np.inf, np.zeros(0, np.int64)
    if len(used):
        xs, ys = X[tri], Y[tri]
        i0 = np.maximum(0, -((-xs.min(axis=1)) // SNAP))
        i1 = np.minimum(nx - 1, xs.max(axis=1) // SNAP)
        j0 = np.maximum(0, -((-ys.min(axis=1)) // SNAP))
        j1 = np.minimum(ny - 1, ys.max(axis=1) // SNAP)
        bw, bh = np.maximum(i1 - i0 + 1, 0), np.maximum(j1 - j0 + 1, 0)
        bw = np.where(bh > 0, bw, 0)
        boxes = bw * bh
        for di in range(int(bw.max())):
            col = np.nonzero(bw > di)[0]
            for dj in range(int(bh[col].max())):
                k = col[bh[col] > dj]
                i, j = i0[k] + di, j0[k] + dj
                px, py = SNAP * i, SNAP * j
                ka, kb, kc_ = a[k], b[k], c[k]
                dxa, dya = X[kc_] - X[kb], Y[kc_] - Y[kb]
                dxb, dyb = X[ka] - X[kc_], Y[ka] - Y[kc_]
                dxc, dyc = X[kb] - X[ka], Y[kb] - Y[ka]
                ea = dxa * (py - Y[kb]) - dya * (px - X[kb])
                eb = dxb * (py - Y[kc_]) - dyb * (px - X[kc_])
                ec = dxc * (py - Y[ka]) - dyc * (px - X[ka])
                sk = s[k]
                own = _edge_in(ea, sk, dxa, dya) & _edge_in(eb, sk, dxb, dyb) & _edge_in(ec, sk, dxc, dyc)
                if not own.any():
                    continue
                k, i, j, ea, eb, ec, sk = (t[own] for t in (k, i, j, ea, eb, ec, sk))
                Ad = area[k].astype(np.float64)
                wa, wb, wc = ea.astype(np.float64) / Ad, eb.astype(np.float64) / Ad, ec.astype(np.float64) / Ad
                with np.errstate(over="ignore"):
                    z = (wa * Z[a[k]] + wb * Z[b[k]]) + wc * Z[c[k]]
                kc = np.clip(np.ceil(z), 0, nz).astype(np.int64)
                np.add.at(count, (i, j, kc), 1)
                np.add.at(signed, (i, j, kc), sk)
                n_cross += len(k)
                vertex_hit = ((ea == 0).astype(int) + (eb == 0) + (ec == 0)) == 2
                rest = z[~vertex_hit & np.isfinite(z)]
                if len(rest):
                    margin = min(margin, float(np.abs(rest - np.rint(rest)).min()))
    # S[m] = the toggles m .. nz; point k looks at S[k + 1], the column at S[0]
    if rule == "parity":
        S = np.cumsum(count[:, :, ::-1], axis=2)[:, :, ::-1] % 2 == 1
    elif rule == "nonzero":
        S = np.cumsum(signed[:, :, ::-1], axis=2)[:, :, ::-1] != 0
    else:
        raise KeyError(rule)
    occ, open_ = S[:, :, 1:], S[:, :, 0]
    stats = np.array([len(used), int(bad.sum()), int(flat.sum()), n_cross, int(open_.sum()), int(occ.sum())], np.int64)
    return dict(occ=occ, bits=pack_bits(occ), stats=stats, open=open_, margin=margin, boxes=boxes, kc=np.nonzero(count.sum(axis=(0, 1)))[0])


def voxel_counts_np(a, b=None):
    """gpnerf_voxel_stats restated on bool cubes -> int64 [4]: A, B, BOTH, EITHER"""
    a = np.asarray(a, bool)
    b = np.zeros_like(a) if b is None else np.asarray(b, bool)
    return np.array([a.sum(), b.sum(), (a & b).sum(), (a | b).sum()], np.int64)


def contains_np(occ, lo, step, points):
    """gpnerf_voxel_contains restated -> uint8 [n]"""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        r = np.rint((p - np.asarray(lo, np.float64)[None]) / np.asarray(step, np.float64)[None])
        inside = np.isfinite(r).all(axis=1) & (r >= 0).all(axis=1) & (r < np.array(occ.shape, np.float64)[None]).all(axis=1)
    idx = np.where(inside[:, None], r, 0).astype(np.int64)
    return (inside & occ[idx[:, 0], idx[:, 1], idx[:, 2]]).astype(np.uint8)


def assert_preconditions(ref):
    assert ref["margin"] > MARGIN, f"a crossing lies within {ref['margin']} of a lattice index: move the mesh"


# ---------------------------------------------------------------- meshes and fields

def box_mesh(lo, hi):
    """the 12 outward-oriented faces of the box lo .. hi"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = mm.f32([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]])
    f = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7]],
                 np.int32)
    return v, f


def join(*meshes):
    vs, fs, n = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32).reshape(-1, 3))
        fs.append(np.asarray(f, np.int64).reshape(-1, 3) + n)
        n += len(vs[-1])
    return mm.f32(np.concatenate(vs)), np.ascontiguousarray(np.concatenate(fs), np.int32)


def placed_sphere(level, radius, centre):
    v, f = mm.icosphere(level)
    return mm.f32(v.astype(np.float64) * np.asarray(radius, np.float64) + np.asarray(centre, np.float64)), f


def mesh_volume(vertices, faces):
    """the divergence theorem's volume of a closed, outward-oriented mesh"""
    t = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float((t[:, 0] * np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def mesh_area(vertices, faces):
    t = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum())


def margined(field, iso=ISO, margin=0.002):
    """the field with every value within `margin` of the iso value pushed to that distance, on its own side"""
    f = np.asarray(field, np.float32).astype(np.float64)
    d = f - float(iso)
    f = np.where(np.abs(d) < margin, float(iso) + np.where(d >= 0, margin, -margin), f)
    return f.astype(np.float32)


@functools.lru_cache(maxsize=None)
def field(name):
    """a cube whose marching-cubes mesh closes inside it: float32, read-only"""
    if name == "sphere":
        f = mesh_cases.sphere_field(n=40, r=12.0)
    elif name == "torus":
        f = mesh_cases.torus_field(n=44, R=11.0, r=4.5)
    elif name == "all_cases":
        f = margined(mesh_cases.all_cases_field())
        assert mesh_cases.case_count(f, ISO) == 256 and (np.abs(f.astype(np.float64) - float(ISO)) >= 0.002 - 1e-7).all()
    else:
        raise KeyError(name)
    assert not (f == ISO).any()
    f.setflags(write=False)
    return f


FIELDS = ("sphere", "torus", "all_cases")


@functools.lru_cache(maxsize=None)
def field_mesh(name):
    """(vertices float32, faces int32) of the restated marching cubes on field(name), in index units"""
    v, f = mesh_cases.marching_cubes_np(field(name), ISO)
    v, f = mm.f32(v), np.ascontiguousarray(f, np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


BOX = ((2.0, 3.0, 1.5), (7.0, 6.0, 5.5))                     # faces exactly on lattice planes in x and y
BOX_B = ((4.0, 4.0, 3.5), (9.0, 9.0, 7.5))                   # 100 points, 12 of them in BOX
LARGE_BOX = 256                                              # columns in a face's box above which the kernels take their second tier
NAMES = ("box_nz9", "box_nz33", "box_nz64", "box_large", "wide_large", "wedge_large", "both_tiers", "all_cases", "degenerate", "outside_xy", "above_below", "twice",
         "two_boxes", "hemisphere", "zero_faces", "anisotropic", "tall")
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _case(name):
    """-> (vertices, faces, lo, step, dims)"""
    if name == "box_nz9":                                     # one partial word; every face in the small tier
        return box_mesh(*BOX) + UNIT + ((12, 10, 9),)
    if name == "box_nz33":                                    # a second word with one bit, which the box reaches
        return box_mesh((2.0, 3.0, 1.5), (7.0, 6.0, 32.5)) + UNIT + ((12, 10, 33),)
    if name == "box_nz64":                                    # the toggle row needs a word more than the output; the lid is above the lattice
        return join(box_mesh((2.0, 3.0, 1.5), (7.0, 6.0, 70.5)), box_mesh((8.0, 1.0, 30.5), (11.0, 4.0, 63.5))) + UNIT + ((12, 10, 64),)
    if name == "box_large":                                   # lid and floor span 30 x 30 columns: the list and its device-side length
        return box_mesh((4.5, 5.5, 2.5), (34.5, 35.5, 16.5)) + UNIT + ((40, 40, 20),)
    if name == "wide_large":                                  # lid and floor span 40 x 9 columns: a box whose two extents differ
        return box_mesh((4.5, 5.5, 2.5), (44.5, 14.5, 16.5)) + UNIT + ((50, 20, 20),)
    if name == "wedge_large":                                 # a tetrahedron: four large faces, none square, every one sloping in z
        v = mm.f32([[3.3, 2.2, 1.5], [45.6, 4.1, 3.5], [20.2, 17.3, 2.5], [22.1, 9.4, 15.5]])
        return (v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)) + UNIT + ((50, 20, 20),)
    if name == "both_tiers":                                  # a sphere of small faces inside the large box, and one beside it
        return join(box_mesh((4.5, 5.5, 2.5), (34.5, 35.5, 16.5)), placed_sphere(2, 6.0, (20.3, 19.7, 10.2)),
                    placed_sphere(1, 1.9, (37.1, 2.3, 5.4))) + UNIT + ((40, 40, 20),)
    if name == "all_cases":                                   # the heaviest: 108 k faces, every marching-cubes case, vertices ON columns
        return field_mesh("all_cases") + UNIT + (field("all_cases").shape,)
    if name == "degenerate":
        # the box, then: a face with no area in projection (vertical), three equal vertices, an index == n_vertices, a negative index,
        # a NaN vertex, an infinite vertex (in z: finite x and y), a vertex beyond the guard band (x = 70 000 steps)
        v, f = box_mesh(*BOX)
        n = len(v)
        v = np.concatenate([v, mm.f32([[3.0, 3.0, 1.0], [3.0, 3.0, 4.0], [np.nan, 1.0, 1.0], [1.0, 1.0, np.inf], [70000.0, 2.0, 2.0]])])
        f = np.concatenate([f, [[n, n + 1, 0], [n, n, n], [0, 1, n + 5], [-1, 2, 3], [0, 1, n + 2], [0, 1, n + 3], [0, 1, n + 4]]])
        return mm.f32(v), np.ascontiguousarray(f, np.int32), UNIT[0], UNIT[1], (12, 10, 9)
    if name == "outside_xy":                                  # boxes wholly outside the lattice in x and in y, and one cut by its border
        return join(box_mesh(*BOX), box_mesh((-20.0, 3.0, 1.5), (-10.0, 6.0, 5.5)), box_mesh((2.0, 10.5, 1.5), (7.0, 16.0, 5.5)),
                    box_mesh((9.5, 7.5, 2.5), (15.0, 12.0, 6.5))) + UNIT + ((12, 10, 9),)
    if name == "above_below":                                 # kc = nz and kc = 0: a box through the whole lattice, a lone face above, one below
        lone = lambda z, x: (mm.f32([[x, 1.2, z], [x + 2.1, 1.4, z], [x + 0.3, 3.7, z]]), np.array([[0, 1, 2]], np.int32))
        return join(box_mesh((2.0, 3.0, -3.5), (7.0, 6.0, 13.5)), lone(11.5, 8.2), lone(-2.5, 8.9)) + UNIT + ((12, 10, 9),)
    if name == "twice":                                       # every face listed twice: cancels under PARITY, counts 2 under NONZERO
        v, f = box_mesh(*BOX)
        return v, np.ascontiguousarray(np.concatenate([f, f[::-1]]), np.int32), UNIT[0], UNIT[1], (12, 10, 9)
    if name == "two_boxes":                                   # 136 points under PARITY (the XOR), 148 under NONZERO (the union)
        return join(box_mesh(*BOX), box_mesh(*BOX_B)) + UNIT + ((12, 12, 9),)
    if name == "hemisphere":                                  # open: the faces of a sphere whose centre lies above its equator
        v, f = placed_sphere(2, 4.3, (6.2, 5.1, 4.4))
        up = v[f][:, :, 2].mean(axis=1) > 4.4
        return v, np.ascontiguousarray(f[up]), UNIT[0], UNIT[1], (12, 10, 9)
    if name == "zero_faces":
        return mm.icosphere(1)[0], np.zeros((0, 3), np.int32), UNIT[0], UNIT[1], (12, 10, 9)
    if name == "anisotropic":                                 # metres: an ellipsoid on a lattice with three steps and an offset origin
        return placed_sphere(3, (0.3, 0.2, 0.5), (0.013, -0.021, 0.007)) + ((-0.41, -0.33, -0.62), (0.02, 0.015, 0.03), (41, 44, 42))
    if name == "tall":                                        # columns of 2100 points: toggle rows of more than 64 words
        return join(box_mesh((-0.5, -0.5, 1.5), (1.5, 2.5, 2050.5)), box_mesh((0.5, 0.5, 100.5), (2.5, 1.5, 2090.5)),
                    placed_sphere(1, (1.1, 1.2, 300.0), (1.03, 0.97, 1200.3))) + UNIT + ((3, 3, 2100),)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, rule):
    """-> dict(v, f, lo, step, dims, ref): the mesh, the lattice, and the restatement's result (computed once, shared, read-only)"""
    v, f, lo, step, dims = _case(name)
    lo, step = np.array(lo, np.float64), np.array(step, np.float64)
    ref = voxelize_np(v, f, lo, step, dims, rule)
    assert_preconditions(ref)
    if name in ("wide_large", "wedge_large"):                 # the case is what it says: every used face goes through the list
        assert len(ref["boxes"]) == 4 and (ref["boxes"] > LARGE_BOX).all(), ref["boxes"]
    if name == "wide_large":
        assert sorted(ref["boxes"].tolist()) == [360] * 4
    if name == "wedge_large":                                 # and a crossing's place is interpolated, not one value per face
        assert sorted(ref["boxes"].tolist()) == sorted([42 * 15, 42 * 7, 25 * 13, 19 * 15]) and len(ref["kc"]) > 4, (ref["boxes"], ref["kc"])
    for a in (v, f, lo, step, ref["occ"], ref["bits"], ref["stats"], ref["open"]):
        a.setflags(write=False)
    return dict(v=v, f=f, lo=lo, step=step, dims=tuple(int(d) for d in dims), ref=ref)
