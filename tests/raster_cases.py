"""The mesh rasteriser (gpnerf_raster.hip) restated in numpy from the text of include/gpnerf_hip.h -- float64 and int64, a brute force
over EVERY face at EVERY pixel, no pixel boxes, no tiers -- and the cases of its tests.  Nothing here looks at what the kernels give.

Both sides evaluate the same unfused float64 expressions on the same float32 inputs, and everything behind the snap to 1/256 pixel is
exact integer arithmetic, so depth bits, face ids and counts are compared for EQUALITY.  The one place where another operation order
could decide differently is the snap itself (rint of 256 x): `case()` asserts of every case it hands out that no snapped coordinate
of a usable vertex lies within hull_cases.TIE_EPS of a half -- the seeds and coordinates below are chosen so that this holds --, so
the comparisons are total and nothing is left out."""
import functools

import numpy as np

import hull_cases
import mesh_metric_cases as mm

GUARD = 2.0 ** 20
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = {"small": (24, 40), "large": (70, 130)}           # (H, W): neither a multiple of 64 lanes nor of a 4 x 8 patch
Z_NEAR = 1e-6


# ---------------------------------------------------------------- the definition

def project(vertices, cam):
    """(x, y, z, usable, X, Y) of float32 vertices [n,3] in one view; X, Y int64 (0 where not usable)"""
    x, y = hull_cases.project_view(np.asarray(vertices, np.float32).astype(np.float64), cam)
    p = np.asarray(vertices, np.float32).astype(np.float64)
    RT, K = cam[9:].reshape(3, 4), cam[:9].reshape(3, 3)
    with np.errstate(all="ignore"):
        c = [((p[:, 0] * RT[r, 0] + p[:, 1] * RT[r, 1]) + p[:, 2] * RT[r, 2]) + RT[r, 3] for r in range(3)]
        z = (c[0] * K[2, 0] + c[1] * K[2, 1]) + c[2] * K[2, 2]
    return x, y, z


def snap(x, y, z, z_near):
    with np.errstate(all="ignore"):
        usable = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z >= z_near) & (np.abs(x) <= GUARD) & (np.abs(y) <= GUARD)
        X = np.where(usable, np.rint(256.0 * np.where(usable, x, 0.0)), 0.0).astype(np.int64)
        Y = np.where(usable, np.rint(256.0 * np.where(usable, y, 0.0)), 0.0).astype(np.int64)
    return usable, X, Y


def face_states(faces, n_vertices, usable, X, Y):
    """(ok index, bad-vertex bool, zero-area bool, doubled area int64) per face"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < n_vertices)).all(axis=1)
    fs = np.where(in_range[:, None], f, 0)
    bad = ~in_range | ~usable[fs].all(axis=1) if n_vertices else np.ones(len(f), bool)
    a, b, c = fs[:, 0], fs[:, 1], fs[:, 2]
    A = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a]) if n_vertices else np.zeros(len(f), np.int64)
    flat = ~bad & (A == 0)
    return fs, bad, flat, A


def edge_functions(X, Y, tri, px, py):
    """Ea, Eb, Ec [faces, pixels] int64 of the faces `tri` [m,3] at pixel centres (px, py) [pixels]"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    col = lambda v: v[:, None]
    ea = col(X[c] - X[b]) * (py[None] - col(Y[b])) - col(Y[c] - Y[b]) * (px[None] - col(X[b]))
    eb = col(X[a] - X[c]) * (py[None] - col(Y[c])) - col(Y[a] - Y[c]) * (px[None] - col(X[c]))
    ec = col(X[b] - X[a]) * (py[None] - col(Y[a])) - col(Y[b] - Y[a]) * (px[None] - col(X[a]))
    return ea, eb, ec


def rasterize_np(vertices, faces, cams, H, W, z_near=Z_NEAR, chunk=128):
    """-> dict(depth float32 [V,H,W], face_id int32 [V,H,W], stats int64 [V,4], keys uint64 [V,H,W])"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    cams = np.asarray(cams, np.float64).reshape(-1, 21)
    n_views = len(cams)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    px, py = 256 * ii.reshape(-1), 256 * jj.reshape(-1)
    keys = np.full((n_views, H * W), EMPTY, np.uint64)
    stats = np.zeros((n_views, 4), np.int64)
    for w in range(n_views):
        x, y, z = project(v, cams[w])
        usable, X, Y = snap(x, y, z, z_near)
        fs, bad, flat, A = face_states(faces, len(v), usable, X, Y)
        drawn = np.nonzero(~bad & ~flat)[0]
        stats[w, :3] = len(drawn), int(bad.sum()), int(flat.sum())
        for s in range(0, len(drawn), chunk):
            idx = drawn[s:s + chunk]
            tri, area = fs[idx], A[idx]
            ea, eb, ec = edge_functions(X, Y, tri, px, py)
            sign = np.sign(area)[:, None]
            cov = (ea * sign >= 0) & (eb * sign >= 0) & (ec * sign >= 0)
            fi, pi = np.nonzero(cov)
            if not len(fi):
                continue
            Ad = area[fi].astype(np.float64)
            wa, wb, wc = ea[fi, pi].astype(np.float64) / Ad, eb[fi, pi].astype(np.float64) / Ad, ec[fi, pi].astype(np.float64) / Ad
            q = (wa / z[tri[fi, 0]] + wb / z[tri[fi, 1]]) + wc / z[tri[fi, 2]]
            with np.errstate(over="ignore", divide="ignore"):
                depth = (1.0 / q).astype(np.float32)
            key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[fi].astype(np.uint64)
            np.minimum.at(keys[w], pi, key)
        stats[w, 3] = int((keys[w] != EMPTY).sum())
    empty = keys == EMPTY
    depth = np.where(empty, np.float32(np.inf), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)).astype(np.float32)
    face_id = np.where(empty, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    sh = (n_views, H, W)
    return dict(depth=depth.reshape(sh), face_id=face_id.reshape(sh), stats=stats, keys=keys.reshape(sh))


def interpolate_np(face_id, vertices, faces, cams, H, W, attrs, background, z_near=Z_NEAR):
    """gpnerf_mesh_interpolate restated -> float32 [V,H,W,C]"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    attrs = np.asarray(attrs, np.float32).reshape(len(v), -1).astype(np.float64)
    C = attrs.shape[1]
    cams = np.asarray(cams, np.float64).reshape(-1, 21)
    out = np.empty((len(cams), H * W, C), np.float32)
    out[:] = np.broadcast_to(np.asarray(background, np.float32), (C,))
    jj, ii = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    px, py = 256 * ii.reshape(-1), 256 * jj.reshape(-1)
    for w in range(len(cams)):
        x, y, z = project(v, cams[w])
        usable, X, Y = snap(x, y, z, z_near)
        fs, bad, flat, A = face_states(faces, len(v), usable, X, Y)
        fid = np.asarray(face_id)[w].reshape(-1).astype(np.int64)
        named = (fid >= 0) & (fid < len(fs))
        pi = np.nonzero(named)[0]
        pi = pi[~bad[fid[pi]] & ~flat[fid[pi]]]
        if not len(pi):
            continue
        tri, area = fs[fid[pi]], A[fid[pi]]
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ea = (X[c] - X[b]) * (py[pi] - Y[b]) - (Y[c] - Y[b]) * (px[pi] - X[b])
        eb = (X[a] - X[c]) * (py[pi] - Y[c]) - (Y[a] - Y[c]) * (px[pi] - X[c])
        ec = (X[b] - X[a]) * (py[pi] - Y[a]) - (Y[b] - Y[a]) * (px[pi] - X[a])
        sign = np.sign(area)
        cov = (ea * sign >= 0) & (eb * sign >= 0) & (ec * sign >= 0)
        pi, a, b, c, ea, eb, ec, area = (t[cov] for t in (pi, a, b, c, ea, eb, ec, area))
        Ad = area.astype(np.float64)
        ta, tb, tc = (ea.astype(np.float64) / Ad) / z[a], (eb.astype(np.float64) / Ad) / z[b], (ec.astype(np.float64) / Ad) / z[c]
        q = (ta + tb) + tc
        ua, ub, uc = ta / q, tb / q, tc / q
        out[w, pi] = ((ua[:, None] * attrs[a] + ub[:, None] * attrs[b]) + uc[:, None] * attrs[c]).astype(np.float32)
    return out.reshape(len(cams), H, W, C)


def silhouette_np(face_id, masks):
    """gpnerf_silhouette_stats restated -> int64 [V,5]: covered, gt, both, either over mask != 100, and the pixels left out"""
    fid, m = np.asarray(face_id), np.asarray(masks, np.uint8)
    out = np.zeros((len(fid), 5), np.int64)
    for w in range(len(fid)):
        keep = m[w] != 100
        cov, gt = (fid[w] >= 0) & keep, (m[w] != 0) & keep
        out[w] = cov.sum(), gt.sum(), (cov & gt).sum(), (cov | gt).sum(), (~keep).sum()
    return out


# ---------------------------------------------------------------- cameras

def look_at(eye, target=(0, 0, 0), up=(0, 0, 1)):
    """RT [3,4] of a camera at `eye` looking at `target`: rows x (right), y (down), z (forward)"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    zc = (target - eye) / np.linalg.norm(target - eye)
    xc = np.cross(zc, up)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    R = np.stack([xc, yc, zc])
    return np.concatenate([R, (-R @ eye)[:, None]], axis=1)


def orbit_cameras(H, W, n_views, radius, distance, seed):
    """n_views cameras around the origin at `distance`, a sphere of `radius` spanning 0.8 of the shorter image side"""
    rng = np.random.default_rng(seed)
    f = 0.4 * min(H, W) * distance / radius
    Ks, RTs = [], []
    for k in range(n_views):
        az, el = 2 * np.pi * (k + rng.uniform(0.1, 0.9)) / n_views, rng.uniform(-0.5, 0.5)
        eye = distance * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
        RTs.append(look_at(eye))
        Ks.append([[f, 0, 0.5 * (W - 1) + rng.uniform(-2, 2)], [0, f * rng.uniform(0.95, 1.05), 0.5 * (H - 1) + rng.uniform(-2, 2)], [0, 0, 1]])
    return np.array(Ks, np.float64), np.array(RTs, np.float64)


def pixel_cameras(n_views):
    """cameras under which a vertex (x z, y z, z) lands on pixel (x, y) exactly in view 0: K = diag(1, 1, 1), RT = [I | 0]; the other
    views scale and shift by dyadic numbers (exact as well)"""
    Ks = np.array([np.diag([s, s, 1.0]) for s in (1.0, 0.75, 1.25, 0.5, 1.5, 0.875, 1.125, 0.625)][:n_views])
    shift = [(0, 0), (2.5, -1.25), (-3.75, 1.5), (1, 1), (-1, 2), (4, 0), (0, -2), (3, 3)][:n_views]
    RTs = np.array([np.concatenate([np.eye(3), [[sx], [sy], [0.0]]], axis=1) for sx, sy in shift])
    return Ks, RTs


def at_pixels(xyz):
    """vertices (x z, y z, z) float32 from rows (x, y, z): pixel positions and depths under pixel_cameras' view 0"""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    return mm.f32(np.stack([p[:, 0] * p[:, 2], p[:, 1] * p[:, 2], p[:, 2]], axis=1))


# ---------------------------------------------------------------- cases

ORBIT = ("one_triangle", "two_triangles", "icosphere2", "icosphere4", "tie_cube", "degenerate_mix", "zero_faces")
PIXEL = ("large_faces", "both_tiers", "near_and_guard", "pixel_centres")
NAMES = ORBIT + PIXEL


def _mesh(name, H, W):
    if name == "one_triangle":
        v, f = mm.one_triangle()
        return mm.f32(v - [0.3, 0.3, 0.0]), f
    if name == "two_triangles":
        v, f = mm.two_triangles()
        return mm.f32(v - [0.5, 0.5, 0.25]), f
    if name.startswith("icosphere"):
        return mm.icosphere(int(name[-1]))
    if name == "tie_cube":
        # every face twice: the coplanar duplicate has, operation for operation, the same depth, and the smaller index wins -- the
        # second copy comes in REVERSED order, so "the first to arrive" and "the smaller index" are different faces
        v, f = mm.tie_cube()
        return mm.f32(0.6 * v), np.ascontiguousarray(np.concatenate([f[::-1], f]), np.int32)
    if name == "degenerate_mix":
        # collinear, three equal vertices, a repeated face (mm.degenerate_mix), then an index == n_vertices, a negative index, and a
        # face with a NaN vertex and one with an infinite vertex
        v, f = mm.degenerate_mix()
        n = len(v)
        v = np.concatenate([0.4 * v, mm.f32([[np.nan, 0, 0], [0, np.inf, 0]])])
        f = np.concatenate([f, [[0, 1, n + 2], [-1, 2, 3], [0, 1, n], [2, n + 1, 3]]]).astype(np.int32)
        return mm.f32(v), np.ascontiguousarray(f)
    if name == "zero_faces":
        return mm.icosphere(1)[0], np.zeros((0, 3), np.int32)
    if name == "large_faces":
        # face 0: larger than the image, every vertex off-screen; face 1: about 340 pixels in a 31 x 24 box (over the 256 of the
        # small tier); face 2: 3 pixels, in front of both
        return at_pixels([[-100.3, -50.2, 2], [3.1 * W, -60.4, 3], [50.6, 6.2 * H, 4],
                          [10.3, 5.2, 1.5], [40.7, 8.1, 1.75], [20.2, 28.6, 1.25],
                          [15.2, 9.9, 1.0], [18.4, 10.3, 1.0], [16.1, 12.7, 1.0]]), np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
    if name == "both_tiers":
        # an icosphere of many small faces in front of a background face that spans the image and a mid-sized one (both listed)
        sv, sf = mm.icosphere(2)
        r = 0.3 * min(H, W)
        sphere = np.stack([0.5 * W + r * sv[:, 0].astype(np.float64), 0.5 * H + r * sv[:, 1].astype(np.float64), 5.0 + sv[:, 2]], axis=1)
        big = [[-40.2, -30.7, 9], [2.6 * W, -20.1, 9.5], [-10.9, 3.3 * H, 8.5], [3.3, 2.1, 7], [0.7 * W, 4.4, 7.5], [5.6, 0.9 * H, 6.5]]
        v = at_pixels(np.concatenate([sphere, big]))
        n = len(sv)
        return v, np.ascontiguousarray(np.concatenate([sf, [[n, n + 1, n + 2], [n + 3, n + 4, n + 5]]]), np.int32)
    if name == "near_and_guard":
        # face 0: fine; face 1: one vertex behind the near plane (z < 0 in view 0); face 2: one vertex at z = z_near / 2; face 3: one
        # vertex beyond the guard band (x > 2^20 pixels); face 4: a vertex at the guard band's edge itself (x = 2^20: usable)
        good = at_pixels([[5.2, 4.1, 2], [30.6, 6.3, 2], [12.4, 20.2, 2]])
        rest = mm.f32([[1.0, 2.0, -1.0], [0.0, 0.0, 0.5 * Z_NEAR], [2.0 ** 21, 3.0, 1.0], [2.0 ** 20, 10.0, 1.0]])
        v = np.concatenate([good, rest])
        return mm.f32(v), np.array([[0, 1, 2], [0, 1, 3], [0, 4, 2], [0, 5, 2], [0, 1, 6]], np.int32)
    if name == "pixel_centres":
        # vertices exactly on pixel centres, edges through pixel centres (the hypotenuse x + y = 12 is shared by faces 0 and 1, at
        # different depths on either side), a horizontal and a vertical edge along pixel rows / columns, a face turned the other way
        # round (face 2: clockwise), and a face that is one pixel centre wide (3)
        v = at_pixels([[2, 2, 1], [10, 2, 2], [2, 10, 4], [10, 10, 1], [20, 3, 2], [28, 3, 2], [24, 15, 1], [30, 20, 2], [31, 20, 2], [30, 21, 2]])
        return v, np.array([[0, 1, 2], [1, 3, 2], [4, 6, 5], [7, 8, 9]], np.int32)
    raise KeyError(name)


def assert_no_near_ties(vertices, faces, cams, z_near=Z_NEAR):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    used = np.zeros(len(v), bool)
    f = np.asarray(faces, np.int64).reshape(-1)
    used[f[(f >= 0) & (f < len(v))]] = True
    for cam in np.asarray(cams, np.float64).reshape(-1, 21):
        x, y, z = project(v, cam)
        usable, _, _ = snap(x, y, z, z_near)
        k = usable & used
        with np.errstate(all="ignore"):
            tie = hull_cases.near_tie(256.0 * x[k]) | hull_cases.near_tie(256.0 * y[k])
        assert not tie.any(), "a snapped coordinate is a near tie: choose another seed"


@functools.lru_cache(maxsize=None)
def case(name, size, n_views):
    """-> dict(v, f, Ks, RTs, cams, H, W, ref): the mesh, the cameras, and the restatement's result (computed once, shared, read-only)"""
    H, W = SIZES[size]
    v, f = _mesh(name, H, W)
    if name in ORBIT:
        Ks, RTs = orbit_cameras(H, W, n_views, radius=1.0, distance=4.0, seed=11 + len(name))
    else:
        Ks, RTs = pixel_cameras(n_views)
    cams = hull_cases.cams_of(Ks, RTs)
    assert_no_near_ties(v, f, cams)
    ref = rasterize_np(v, f, cams, H, W)
    for a in list(ref.values()) + [v, f, Ks, RTs, cams]:
        a.setflags(write=False)
    return dict(v=v, f=f, Ks=Ks, RTs=RTs, cams=cams, H=H, W=W, ref=ref)


def colours_of(vertices, channels, seed=3):
    """float32 attributes [n, channels] in [0, 1]"""
    return mm.f32(np.random.default_rng(seed).uniform(0, 1, (len(vertices), channels)))
