"""Fixtures and the numpy restatement for the registration tests (gpnerf_align.hip; include/gpnerf_hip.h states the definitions restated
here): the strided and tree summation, Horn's matrix and the cyclic Jacobi, the Cholesky solve, the Cayley update, the composition
and transform_points -- operation for operation in float64 (Python floats for the one-thread parts: the same IEEE operations).
Nothing here looks at what the kernels give.
"""
import math

import numpy as np

import mesh_metric_cases as mc

THREADS, BLOCKS = 256, 64                                  # include/gpnerf_hip.h GPNERF_ALIGN_THREADS / _BLOCKS
OK, FEW, SINGULAR = 0, 1, 2
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


# ---------------------------------------------------------------- the sums

def strided_tree_sum(terms):
    """terms float64 [n, K] (a pair that is not used: a row of zeros) -> [K]: thread t of workgroup b adds the pairs
    (k BLOCKS + b) THREADS + t in ascending k onto zero; 256 partials fold by x[t] += x[t + s], s = 128 .. 1; the 64 rows by the
    same tree from s = 32"""
    terms = np.asarray(terms, np.float64)
    n, K = terms.shape
    per = THREADS * BLOCKS
    rounds = max(1, -(-n // per))
    padded = np.zeros((rounds * per, K))
    padded[:n] = terms
    padded = padded.reshape(rounds, BLOCKS, THREADS, K)
    acc = np.zeros((BLOCKS, THREADS, K))
    for k in range(rounds):
        acc = acc + padded[k]
    s = THREADS // 2
    while s:
        acc = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    rows = acc[:, 0]
    s = BLOCKS // 2
    while s:
        rows = rows[:s] + rows[s:2 * s]
        s //= 2
    return rows[0]


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---------------------------------------------------------------- the one-thread parts (Python floats)

def quat_to_R(q):
    w, x, y, z = (float(v) for v in q)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
            [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
            [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]


def jacobi4(A):
    """cyclic Jacobi, 8 sweeps, on a symmetric 4 x 4 (lists of Python floats) -> (A, V): V's columns are the eigenvectors"""
    A = [[float(v) for v in row] for row in A]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(8):
        for p in range(3):
            for q in range(p + 1, 4):
                if A[p][q] == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                den = abs(theta) + math.sqrt(theta * theta + 1.0)
                t = -1.0 / den if theta < 0.0 else 1.0 / den
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
                for k in range(4):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
                A[p][q] = A[q][p] = 0.0
                for k in range(4):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    return A, V


def horn_matrix(S):
    S = [float(v) for v in S]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (S[0] + S[4]) + S[8]
    N[1][1] = (S[0] - S[4]) - S[8]
    N[2][2] = (S[4] - S[0]) - S[8]
    N[3][3] = (S[8] - S[0]) - S[4]
    N[0][1] = N[1][0] = S[5] - S[7]
    N[0][2] = N[2][0] = S[6] - S[2]
    N[0][3] = N[3][0] = S[1] - S[3]
    N[1][2] = N[2][1] = S[1] + S[3]
    N[1][3] = N[3][1] = S[6] + S[2]
    N[2][3] = N[3][2] = S[5] + S[7]
    return N


def horn_solve(S, saa, c_src, c_dst, with_scale):
    """(status, M [3,4], scale) from the centred sums: what gpnerf_rigid_fit's solving thread does behind the FEW test"""
    if not (saa > 0.0) or not math.isfinite(saa):
        return SINGULAR, IDENTITY.copy(), 1.0
    A, V = jacobi4(horn_matrix(S))
    best = 0
    for j in range(1, 4):
        if A[j][j] > A[best][best]:
            best = j
    if A[0][0] == A[1][1] == A[2][2] == A[3][3]:
        return SINGULAR, IDENTITY.copy(), 1.0
    q = [V[k][best] for k in range(4)]
    length = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [v / length for v in q]
    if q[0] < 0.0:
        q = [-v for v in q]
    R = quat_to_R(q)
    scale = 1.0
    if with_scale:
        num = 0.0
        for i in range(3):
            for j in range(3):
                num += R[i][j] * float(S[3 * j + i])
        scale = num / saa
    M = np.zeros((3, 4))
    cs, cd = [float(v) for v in c_src], [float(v) for v in c_dst]
    for i in range(3):
        for j in range(3):
            M[i, j] = scale * R[i][j]
        M[i, 3] = cd[i] - scale * ((R[i][0] * cs[0] + R[i][1] * cs[1]) + R[i][2] * cs[2])
    if not (math.isfinite(scale) and scale > 0.0 and np.isfinite(M).all()):
        return SINGULAR, IDENTITY.copy(), 1.0
    return OK, M, scale


def rigid_fit(src, dst, weights=None, with_scale=False):
    """gpnerf_rigid_fit restated -> dict: status, M [3,4], scale, used, skipped, wsum, rms, pivot, and the sums the workspace
    shows: sums1 [7], centroids [6], sums2 [11]"""
    a, b = _f64(src).reshape(-1, 3), _f64(dst).reshape(-1, 3)
    n = len(a)
    w = np.ones(n) if weights is None else _f64(weights).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(w) & (w > 0)
    used, skipped = int(ok.sum()), int(n - ok.sum())
    a, b, w = np.where(ok[:, None], a, 0.0), np.where(ok[:, None], b, 0.0), np.where(ok, w, 0.0)
    sums1 = strided_tree_sum(np.concatenate([w[:, None], w[:, None] * a, w[:, None] * b], axis=1))
    cen = sums1[1:] / sums1[0] if used > 0 else np.zeros(6)
    ca, cb, e = a - cen[:3], b - cen[3:], b - a
    wa = w[:, None] * ca
    terms = np.concatenate([(wa[:, :, None] * cb[:, None, :]).reshape(n, 9), (w * _dot(ca, ca))[:, None], (w * _dot(e, e))[:, None]], axis=1)
    sums2 = strided_tree_sum(np.where(ok[:, None], terms, 0.0))
    if used < 3:
        status, M, scale = FEW, IDENTITY.copy(), 1.0
    else:
        status, M, scale = horn_solve(sums2[:9], float(sums2[9]), cen[:3], cen[3:], with_scale)
    rms = math.sqrt(float(sums2[10]) / float(sums1[0])) if used > 0 else float("nan")
    return {"status": status, "M": M, "scale": scale, "used": used, "skipped": skipped, "wsum": float(sums1[0]), "rms": rms,
            "pivot": cen[:3].copy(), "sums1": sums1, "centroids": cen, "sums2": sums2}


def pivot_of(points):
    """gpnerf_align_init's PIVOT: the unweighted centroid of the finite points, in the fixed order"""
    p = _f64(points).reshape(-1, 3)
    ok = np.isfinite(p).all(axis=1)
    if not ok.any():
        return np.zeros(3)
    s = strided_tree_sum(np.concatenate([ok[:, None].astype(np.float64), np.where(ok[:, None], p, 0.0)], axis=1))
    return s[1:] / s[0]


def transform_points(points, M, scale=1.0, vectors=False):
    """gpnerf_transform_points restated: float32 [n,3]"""
    p = _f64(points).reshape(-1, 3)
    M = np.asarray(M, np.float64).reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        if vectors:
            m = M[:, :3] / float(scale)
            out = np.stack([(m[k, 0] * p[:, 0] + m[k, 1] * p[:, 1]) + m[k, 2] * p[:, 2] for k in range(3)], axis=1)
        else:
            out = np.stack([((M[k, 0] * p[:, 0] + M[k, 1] * p[:, 1]) + M[k, 2] * p[:, 2]) + M[k, 3] for k in range(3)], axis=1)
        out = out.astype(np.float32)
    out[~np.isfinite(p).all(axis=1)] = np.nan
    return out


def cholesky_solve6(A, g):
    """(status, x): the header's column-by-column Cholesky with its pivot rule; A [6,6] symmetric, g [6]"""
    A = [[float(v) for v in row] for row in np.asarray(A)]
    g = [float(v) for v in g]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        dj = A[j][j]
        for k in range(j):
            dj = dj - L[j][k] * L[j][k]
        if not (dj > 2.0 ** -30 * A[j][j]):
            return SINGULAR, None
        L[j][j] = math.sqrt(dj)
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = g[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    return OK, x


def pivot_image(M, pivot):
    c = [float(v) for v in pivot]
    return [((float(M[k, 0]) * c[0] + float(M[k, 1]) * c[1]) + float(M[k, 2]) * c[2]) + float(M[k, 3]) for k in range(3)]


def step_update(M, pivot, x):
    """the Cayley rotation of x[:3], the translation x[3:], about c' = M pivot, composed onto M on the left -> M' [3,4]"""
    h = [x[0] / 2.0, x[1] / 2.0, x[2] / 2.0]
    inv = 1.0 / math.sqrt(1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]))
    R = quat_to_R([inv, h[0] * inv, h[1] * inv, h[2] * inv])
    cp = pivot_image(M, pivot)
    ts = [(cp[i] + x[3 + i]) - ((R[i][0] * cp[0] + R[i][1] * cp[1]) + R[i][2] * cp[2]) for i in range(3)]
    out = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            v = (R[i][0] * float(M[0, j]) + R[i][1] * float(M[1, j])) + R[i][2] * float(M[2, j])
            if j == 3:
                v = v + ts[i]
            out[i, j] = v
    return out


def align_step(cur, closest, face, dist, vertices, faces, max_dist, M, pivot):
    """gpnerf_align_step restated -> dict: status, M (the composed matrix; the one given when the status is not OK), used, skipped,
    trimmed, rms, sums [29], x (the solution, None unless OK)"""
    p, q = _f64(cur).reshape(-1, 3), _f64(closest).reshape(-1, 3)
    d = np.asarray(dist, np.float32).reshape(-1)
    f = np.asarray(face, np.int64).reshape(-1)
    v, fa = np.asarray(vertices, np.float32), np.asarray(faces, np.int64)
    M = np.asarray(M, np.float64).reshape(3, 4)
    n = len(p)
    with np.errstate(invalid="ignore"):
        skip = np.isnan(d) | ~np.isfinite(p).all(axis=1)
        trim = ~skip & (d > np.float32(max_dist))
        rest = ~skip & ~trim
        bad = rest & ((f < 0) | (f >= len(fa)) | ~np.isfinite(d) | ~np.isfinite(q).all(axis=1))
        cand = rest & ~bad
        cand[cand] &= mc.valid_faces(v, fa[f[cand]])
        nf = np.zeros((n, 3))
        length = np.zeros(n)
        tri = v.astype(np.float64)[fa[f[cand]]]
        nn = _cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        length[cand] = np.sqrt(_dot(nn, nn))
        nf[cand] = nn
        use = cand & (length > 0) & np.isfinite(length)
        nf = np.where(use[:, None], nf / np.where(use, length, 1.0)[:, None], 0.0)
    used, trimmed = int(use.sum()), int(trim.sum())
    skipped = n - used - trimmed
    cp = np.array(pivot_image(M, pivot))
    pz, qz = np.where(use[:, None], p, 0.0), np.where(use[:, None], q, 0.0)
    J = np.concatenate([_cross(pz - cp, nf), nf], axis=1)
    r = _dot(qz - pz, nf)
    cols = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)] + [r * r, use.astype(np.float64)]
    sums = strided_tree_sum(np.where(use[:, None], np.stack(cols, axis=1), 0.0))
    rms = math.sqrt(float(sums[27]) / float(sums[28])) if used > 0 else float("nan")
    res = {"status": OK, "M": M.copy(), "used": used, "skipped": skipped, "trimmed": trimmed, "rms": rms, "sums": sums, "x": None}
    if used < 6:
        res["status"] = FEW
        return res
    A = np.zeros((6, 6))
    at = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = sums[at]
            at += 1
    status, x = cholesky_solve6(A, sums[21:27])
    res["A"] = A
    if status == OK:
        Mn = step_update(M, pivot, x)
        if np.isfinite(Mn).all():
            res["M"], res["x"] = Mn, x
        else:
            status = SINGULAR
    res["status"] = status
    return res


def correspondences(cur, vertices, faces, max_dist=np.inf):
    """what gpnerf_mesh_distance writes for float32 queries, from mesh_metric_cases' float32 restatement: (closest float32 [n,3],
    face int32 [n], dist float32 [n])"""
    cur = np.asarray(cur, np.float32)
    v, f = np.asarray(vertices, np.float32), np.asarray(faces, np.int64)
    dist, face = mc.nearest(cur, v, f, np.float32, max_dist)
    hit = face >= 0
    closest = np.full((len(cur), 3), np.nan, np.float32)
    tri = v[f[face[hit]]]
    cp = mc.closest_on_triangle(cur[hit], tri[:, 0], tri[:, 1], tri[:, 2], np.float32)[0]
    closest[hit] = cur[hit] + cp
    return closest, face.astype(np.int32), dist.astype(np.float32)


def icp(points, vertices, faces, iterations=10, max_dist=np.inf, init=None):
    """frame.align_mesh's loop on given source points, restated: align_init, then per iteration transform_points from the ORIGINAL
    points, the nearest points, align_step -> (M [3,4], history [iterations, 4], pivot)"""
    M = IDENTITY.copy() if init is None else np.asarray(init, np.float64).reshape(3, 4).copy()
    pivot = pivot_of(points)
    history = np.zeros((iterations, 4))
    for it in range(iterations):
        cur = transform_points(points, M)
        closest, face, dist = correspondences(cur, vertices, faces)
        step = align_step(cur, closest, face, dist, vertices, faces, max_dist, M, pivot)
        M = step["M"]
        history[it] = step["rms"], step["used"], step["trimmed"], step["status"]
    return M, history, pivot


# ---------------------------------------------------------------- fixtures

def rotation(axis, degrees):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(degrees)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def ellipsoid(centre=(0.0, 0.0, 0.0)):
    """icosphere(3) scaled by (1.0, 0.7, 0.5): 1 280 faces"""
    v, f = mc.icosphere(3)
    return mc.f32(v.astype(np.float64) * np.array([1.0, 0.7, 0.5]) + np.asarray(centre, np.float64)), f


OFF_CENTRE = (10.0, -5.0, 3.0)
# (rotation in degrees about the ellipsoid's centre, shift): the misplacements the loop has to undo
MISPLACEMENTS = {"15deg": ((1.0, 2.0, -1.0), 15.0, (0.1, -0.05, 0.03)), "30deg": ((-1.0, 0.5, 2.0), 30.0, (0.2, 0.1, -0.1))}


def misplacement(name, centre):
    """(A [3,4] float64: x -> R (x - centre) + centre + shift, and its inverse, the transform the loop should find)"""
    axis, deg, shift = MISPLACEMENTS[name]
    R, c, s = rotation(axis, deg), np.asarray(centre, np.float64), np.asarray(shift, np.float64)
    A = np.hstack([R, (c + s - R @ c)[:, None]])
    inv = np.hstack([R.T, (-R.T @ A[:, 3])[:, None]])
    return A, inv


def apply(M, p):
    M = np.asarray(M, np.float64).reshape(3, 4)
    return np.asarray(p, np.float64) @ M[:, :3].T + M[:, 3]


def surface_samples(vertices, faces, n, seed=0):
    """n stratified area-weighted float32 points on the mesh (the header's sampling rule, through mesh_metric_cases)"""
    prefix = np.cumsum(mc.face_areas(vertices, faces))
    target = (np.arange(n) + 0.5) / n * prefix[-1]
    face_of = np.minimum(np.searchsorted(prefix, target, side="right"), len(faces) - 1)
    return mc.sample_points_np(vertices, faces, face_of, seed, np.float32)


def icp_case(name, n=1000, outliers=False):
    """(source points float32 [n,3], the mesh (v, f), M_true [3,4]) of a loop case on the off-centre ellipsoid: surface samples,
    misplaced; outliers: every tenth one moved by +3 on each axis"""
    v, f = ellipsoid(OFF_CENTRE)
    A, inv = misplacement(name, OFF_CENTRE)
    pts = apply(A, surface_samples(v, f, n, seed=3).astype(np.float64))
    if outliers:
        pts[::10] += 3.0
    return mc.f32(pts), (v, f), inv


def loop_bound(points):
    """2^-18 max |coordinate|: about 30 x the float32 query's floor"""
    return 2.0 ** -18 * float(np.abs(np.asarray(points, np.float64)).max())


def pair_set(n, seed, weights=False, dirty=False, scale=1.0):
    """n anisotropic random pairs: dst = s R src + t + noise.  dirty: some NaN coordinates, zero and negative weights"""
    rng = np.random.default_rng(seed)
    src = rng.normal(size=(n, 3)) * np.array([1.0, 0.6, 0.3]) + np.array([0.5, -1.0, 2.0])
    R = rotation(rng.normal(size=3), rng.uniform(5, 170))
    dst = scale * src @ R.T + rng.normal(size=3) + rng.normal(size=(n, 3)) * 0.01
    w = rng.uniform(0.25, 2.0, n).astype(np.float32) if weights or dirty else None
    src, dst = mc.f32(src), mc.f32(dst)
    if dirty and n:
        idx = np.arange(n)
        src[idx % 7 == 3, 1] = np.nan
        dst[idx % 11 == 5, 2] = np.inf
        w[idx % 5 == 4] = 0.0
        w[idx % 13 == 6] = -1.0
        w[idx % 17 == 9] = np.nan
    return src, dst, w


def kabsch(src, dst, w=None, with_scale=False):
    """the reference: SVD-Kabsch / Umeyama from numpy.linalg on the valid pairs -> (R, t, s)"""
    a, b = _f64(src), _f64(dst)
    w = np.ones(len(a)) if w is None else _f64(w)
    ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(w) & (w > 0)
    a, b, w = a[ok], b[ok], w[ok]
    ca, cb = (w[:, None] * a).sum(0) / w.sum(), (w[:, None] * b).sum(0) / w.sum()
    H = ((a - ca) * w[:, None]).T @ (b - cb)
    U, D, Vt = np.linalg.svd(H)
    sign = np.sign(np.linalg.det(Vt.T @ U.T))
    E = np.diag([1.0, 1.0, sign])
    R = Vt.T @ E @ U.T
    s = float((D * np.diag(E)).sum() / (w * ((a - ca) ** 2).sum(1)).sum()) if with_scale else 1.0
    return R, cb - s * R @ ca, s


def eigen_gap(src, dst, w=None):
    """(top eigenvalue gap of Horn's matrix) / (largest |eigenvalue|), and the condition number of the source scatter"""
    r = rigid_fit(src, dst, w)
    ev = np.linalg.eigvalsh(np.array(horn_matrix(r["sums2"][:9])))
    a = _f64(src)
    ok = np.isfinite(a).all(axis=1)
    sc = np.linalg.eigvalsh(np.cov((a[ok] - a[ok].mean(0)).T))
    return float((ev[-1] - ev[-2]) / np.abs(ev).max()), float(sc[-1] / max(sc[0], 1e-300))
