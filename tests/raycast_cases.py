"""Meshes, ray sets and the numpy restatements for the ray-casting tests (gpnerf_raycast.hip; include/gpnerf_hip.h states the
definitions restated here: THE INTERSECTION, the result of a ray, THE WALK and gpnerf_pixel_rays).

`intersect(rays, a, b, c, dtype)` is THE INTERSECTION, operation for operation, vectorised: run in float32 it is what the kernels
must give bit for bit; run in float64 on the same float32 inputs it is the reference of the accuracy bound (4 x the float32
restatement's own deviation from it).  `closest_hit` is the brute force over all faces with the tie rule.  `walk_cells` restates THE
WALK and `dda_cells` an exact Amanatides-Woo walk, over a grid entered on the host (`host_grid`), for counting cells and for showing
what a walk without margins loses.  Nothing here looks at what the kernels give.
"""
import functools

import numpy as np

import mesh_metric_cases as mc
from mesh_metric_cases import f32, valid_faces

INF = np.float32(np.inf)


# ---------------------------------------------------------------- THE INTERSECTION

def _pick(v, k):
    """v[..., k] for an index array k broadcast against v's leading dimensions"""
    return np.take_along_axis(v, np.broadcast_to(k[..., None], v.shape[:-1] + (1,)), axis=-1)[..., 0]


def ray_axes(d):
    """(kx, ky, kz, Sx, Sy, Sz) of directions d [n,3], in d's dtype"""
    ad = np.abs(d)
    kz = np.zeros(len(d), np.int64)
    kz[ad[:, 1] > ad[:, 0]] = 1
    kz[ad[:, 2] > np.maximum(ad[:, 0], ad[:, 1])] = 2
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    dz = _pick(d, kz)
    swap = dz < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(divide="ignore", invalid="ignore"):
        return kx, ky, kz, _pick(d, kx) / dz, _pick(d, ky) / dz, (d.dtype.type(1) / dz)


def ray_valid(rays):
    r = np.asarray(rays, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(r[:, :6]).all(axis=1) & (r[:, 3:6] != 0).any(axis=1) & (r[:, 6] <= r[:, 7])


def intersect(rays, a, b, c, dtype=np.float32):
    """rays [n,8] against faces a, b, c [m,3] -> (hit [n,m] bool, t, wb, wc [n,m] in dtype; garbage where not hit)"""
    r = np.asarray(rays, np.float32).astype(dtype)
    a, b, c = (np.asarray(x, np.float32).astype(dtype)[None] for x in (a, b, c))
    o, d, tmin, tmax = r[:, None, 0:3], r[:, 3:6], r[:, 6, None], r[:, 7, None]
    kx, ky, kz, Sx, Sy, Sz = ray_axes(d)
    kx, ky, kz, Sx, Sy, Sz = (x[:, None] for x in (kx, ky, kz, Sx, Sy, Sz))

    def shear(v):
        V = v - o
        vz = _pick(V, kz)
        return _pick(V, kx) - Sx * vz, _pick(V, ky) - Sy * vz, Sz * vz

    with np.errstate(all="ignore"):
        Ax, Ay, Az = shear(a)
        Bx, By, Bz = shear(b)
        Cx, Cy, Cz = shear(c)
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        assert U.dtype == dtype
        z = (U == 0) | (V == 0) | (W == 0)
        miss = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        if z.any():
            w = lambda x: x[z].astype(np.float64)
            Ud, Vd, Wd = w(Cx) * w(By) - w(Cy) * w(Bx), w(Ax) * w(Cy) - w(Ay) * w(Cx), w(Bx) * w(Ay) - w(By) * w(Ax)
            miss[z] = ((Ud < 0) | (Vd < 0) | (Wd < 0)) & ((Ud > 0) | (Vd > 0) | (Wd > 0))
            U[z], V[z], W[z] = Ud.astype(dtype), Vd.astype(dtype), Wd.astype(dtype)
        det = (U + V) + W
        T = (U * Az + V * Bz) + W * Cz
        t = T / det
        hit = ~miss & (det != 0) & (t >= tmin) & (t <= tmax)
        return hit, t, V / det, W / det


def closest_hit(rays, vertices, faces, dtype=np.float32, chunk=1 << 21):
    """the result of every ray: (t [n], face [n], bary [n,2], hits [n] = the number of faces accepted), t and bary in dtype"""
    rays, v, f = np.asarray(rays, np.float32), np.asarray(vertices, np.float32), np.asarray(faces, np.int64)
    fv = f[valid_faces(v, f)]
    index = np.flatnonzero(valid_faces(v, f))
    n = len(rays)
    t_out, face = np.full(n, np.inf, dtype), np.full(n, -1, np.int64)
    bary, hits = np.full((n, 2), np.nan, dtype), np.zeros(n, np.int64)
    ok = ray_valid(rays)
    rows = max(1, chunk // max(1, len(fv)))
    for i in range(0, n, rows):
        sel = np.flatnonzero(ok[i:i + rows]) + i
        if not len(sel) or not len(fv):
            continue
        hit, t, wb, wc = intersect(rays[sel], v[fv[:, 0]], v[fv[:, 1]], v[fv[:, 2]], dtype)
        t = np.where(hit, t, np.inf)
        j = t.argmin(axis=1)                                     # (the first of the smallest: the lowest face index)
        any_hit = hit.any(axis=1)
        rows_ = np.arange(len(sel))
        t_out[sel] = np.where(any_hit, t[rows_, j], np.inf)
        face[sel] = np.where(any_hit, index[j], -1)
        bary[sel, 0] = np.where(any_hit, wb[rows_, j], np.nan)
        bary[sel, 1] = np.where(any_hit, wc[rows_, j], np.nan)
        hits[sel] = hit.sum(axis=1)
    t_out[~ok] = np.nan
    return t_out, face, bary, hits


def edge_function(px, py, qx, qy):
    """f(P, Q) of THE INTERSECTION in the arguments' dtype"""
    return px * qy - py * qx


# ---------------------------------------------------------------- gpnerf_pixel_rays

def invert3(m):
    m = [float(x) for x in np.asarray(m, np.float64).ravel()]
    c = [m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
         m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
         m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]
    det = (m[0] * c[0] + m[1] * c[3]) + m[2] * c[6]
    return np.array([x / det for x in c], np.float64).reshape(3, 3)


def pixel_rays(Ks, RTs, H, W, z_near=1e-6):
    """gpnerf_pixel_rays restated: float32 [n,H,W,8]"""
    Ks, RTs = np.asarray(Ks, np.float64).reshape(-1, 3, 3), np.asarray(RTs, np.float64).reshape(-1, 3, 4)
    out = np.empty((len(Ks), H, W, 8), np.float32)
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for n, (K, RT) in enumerate(zip(Ks, RTs)):
        Ki, Ri, T = invert3(K), invert3(RT[:, :3]), RT[:, 3]
        c = [(Ki[r, 0] * col + Ki[r, 1] * row) + Ki[r, 2] for r in range(3)]
        u, v = c[0] / c[2], c[1] / c[2]
        for a in range(3):
            out[n, :, :, a] = np.float32(-((Ri[a, 0] * T[0] + Ri[a, 1] * T[1]) + Ri[a, 2] * T[2]))
            out[n, :, :, 3 + a] = ((Ri[a, 0] * u + Ri[a, 1] * v) + Ri[a, 2]).astype(np.float32)
        out[n, :, :, 6] = np.float32(z_near)
        out[n, :, :, 7] = np.inf
    return out


def look_at(eye, target, H, W, focal):
    """(K [3,3], RT [3,4]) of a pinhole camera at `eye` looking at `target`, float64"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    K = np.array([[focal, 0, (W - 1) / 2], [0, focal, (H - 1) / 2], [0, 0, 1]], np.float64)
    return K, np.concatenate([R, (-R @ eye)[:, None]], axis=1)


# ---------------------------------------------------------------- THE WALK, on a grid entered on the host

def cell_of(x, lo, inv, n):
    """the grid's cell function, float32"""
    x, lo, inv = np.float32(x), np.float32(lo), np.float32(inv)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((x - lo) * inv)
    return np.minimum(np.maximum(t, np.float32(0)), np.float32(n - 1)).astype(np.int64)


def host_grid(vertices, faces, cells):
    """a grid of `cells` = (nx, ny, nz) cells over the valid faces' box, entered the way the build enters it (its own cell function;
    size and inv as the build derives them from the box): {"lo", "size", "inv", "n", "cells": {cell index: [faces, ascending]}, "span"}"""
    v, f = np.asarray(vertices, np.float32), np.asarray(faces, np.int64)
    ok = valid_faces(v, f)
    tri = v[f[ok]]
    lo, hi = tri.min(axis=(0, 1)), tri.max(axis=(0, 1))
    n = np.asarray(cells, np.int64)
    w = ((hi.astype(np.float64) - lo.astype(np.float64)) / n).astype(np.float32)
    size = np.where((w > 0) & np.isfinite(w), w, np.float32(1)).astype(np.float32)
    inv = (np.float32(1) / size).astype(np.float32)
    c0 = np.stack([cell_of(tri.min(axis=1)[:, k], lo[k], inv[k], n[k]) for k in range(3)], axis=1)
    c1 = np.stack([cell_of(tri.max(axis=1)[:, k], lo[k], inv[k], n[k]) for k in range(3)], axis=1)
    table = {}
    for face, a, b in zip(np.flatnonzero(ok), c0, c1):
        for cx in range(a[0], b[0] + 1):
            for cy in range(a[1], b[1] + 1):
                for cz in range(a[2], b[2] + 1):
                    table.setdefault((cx * n[1] + cy) * n[2] + cz, []).append(int(face))
    return {"lo": lo, "size": size, "inv": inv, "n": n, "cells": table, "span": (c1 - c0).max(axis=0) if len(c0) else np.zeros(3, np.int64)}


def walk_cells(ray, grid, best_of=None):
    """THE WALK of one valid ray restated in float64: the list of cell indices in visiting order.  best_of(cell) -> the smallest t
    accepted in that cell's faces (or inf), for the early stop; None walks to the end."""
    r = np.asarray(ray, np.float32).astype(np.float64)
    o, d, tmin, tmax = r[0:3], r[3:6], r[6], r[7]
    lo, cs, n = grid["lo"].astype(np.float64), grid["size"].astype(np.float64), grid["n"]
    rho, drho = (o - lo) / cs, d / cs
    R = max(abs(o[a] - lo[a]) + 1.001 * n[a] * cs[a] for a in range(3))
    pad = 2.0 ** -20 * R / cs + 2.0 ** -11
    b0, b1 = -np.inf, np.inf
    for a in range(3):
        l, h = -pad[a], n[a] + pad[a]
        if drho[a] == 0:
            if rho[a] < l or rho[a] > h:
                return []
        else:
            sa, sb = (l - rho[a]) / drho[a], (h - rho[a]) / drho[a]
            b0, b1 = max(b0, min(sa, sb)), min(b1, max(sa, sb))
    if not b0 <= b1:
        return []
    ad = np.abs(np.asarray(ray, np.float32)[3:6])
    az = 0
    if ad[1] > ad[0]:
        az = 1
    if ad[2] > max(ad[0], ad[1]):
        az = 2
    ax, ay = (az + 1) % 3, (az + 2) % 3
    stride = (n[1] * n[2], n[2], 1)
    up = drho[az] > 0
    z0, dzeta, span = (rho[az] if up else n[az] - rho[az]), abs(drho[az]), float(grid["span"][az])
    with np.errstate(invalid="ignore"):
        first = max(np.floor(z0 + b0 * dzeta - pad[az]), np.floor(z0 + tmin * dzeta - pad[az]) - span, 0.0)
        last = min(np.floor(z0 + b1 * dzeta + pad[az]), float(n[az] - 1))
    out, best = [], np.inf
    if not first <= last:
        return out
    clamp = lambda x, m: int(min(max(np.floor(x), 0.0), m - 1))
    for j in range(int(first), int(last) + 1):
        if j > np.floor(z0 + min(tmax, best) * dzeta + pad[az]) + span:
            break
        c = j if up else n[az] - 1 - j
        sa, sb = (c - 2.0 ** -11 - rho[az]) / drho[az], (c + 1 + 2.0 ** -11 - rho[az]) / drho[az]
        xa, xb, ya, yb = rho[ax] + sa * drho[ax], rho[ax] + sb * drho[ax], rho[ay] + sa * drho[ay], rho[ay] + sb * drho[ay]
        for cx in range(clamp(min(xa, xb) - pad[ax], n[ax]), clamp(max(xa, xb) + pad[ax], n[ax]) + 1):
            for cy in range(clamp(min(ya, yb) - pad[ay], n[ay]), clamp(max(ya, yb) + pad[ay], n[ay]) + 1):
                cell = int(c * stride[az] + cx * stride[ax] + cy * stride[ay])
                out.append(cell)
                if best_of is not None:
                    best = min(best, best_of(cell))
    return out


def dda_cells(ray, grid):
    """an EXACT walk without margins (Amanatides and Woo, float64): the cells the real ray passes through inside the box, in order"""
    r = np.asarray(ray, np.float32).astype(np.float64)
    o, d, tmin, tmax = r[0:3], r[3:6], r[6], r[7]
    lo, cs, n = grid["lo"].astype(np.float64), grid["size"].astype(np.float64), grid["n"]
    t0, t1 = tmin, tmax
    for a in range(3):
        if d[a] == 0:
            if o[a] < lo[a] or o[a] > lo[a] + n[a] * cs[a]:
                return []
        else:
            sa, sb = (lo[a] - o[a]) / d[a], (lo[a] + n[a] * cs[a] - o[a]) / d[a]
            t0, t1 = max(t0, min(sa, sb)), min(t1, max(sa, sb))
    if not t0 <= t1:
        return []
    p = o + t0 * d
    c = [int(min(max(np.floor((p[a] - lo[a]) / cs[a]), 0), n[a] - 1)) for a in range(3)]
    step = [1 if d[a] > 0 else -1 for a in range(3)]
    nxt = [((lo[a] + (c[a] + (step[a] > 0)) * cs[a] - o[a]) / d[a]) if d[a] != 0 else np.inf for a in range(3)]
    out = []
    while all(0 <= c[a] < n[a] for a in range(3)):
        out.append(int((c[0] * n[1] + c[1]) * n[2] + c[2]))
        a = int(np.argmin(nxt))
        if nxt[a] > t1:
            break
        c[a] += step[a]
        nxt[a] = (lo[a] + (c[a] + (step[a] > 0)) * cs[a] - o[a]) / d[a]
    return out


def cast_through(ray, vertices, faces, grid, cells):
    """the nearest hit of one ray over the faces of the given cells, float32 restatement: (t, face)"""
    fs = sorted({f for c in cells for f in grid["cells"].get(c, ())})
    if not fs:
        return np.float32(np.inf), -1
    sub = np.asarray(faces, np.int64)[fs]
    t, face, _, _ = closest_hit(np.asarray(ray, np.float32)[None], vertices, sub)
    return t[0], (fs[face[0]] if face[0] >= 0 else -1)


# ---------------------------------------------------------------- rays

def rays_of(o, d, tmin=0.0, tmax=np.inf):
    o, d = np.broadcast_arrays(np.asarray(o, np.float64), np.asarray(d, np.float64))
    r = np.empty(o.shape[:-1] + (8,), np.float32)
    r[..., 0:3], r[..., 3:6] = o, d
    r[..., 6], r[..., 7] = tmin, tmax
    return r.reshape(-1, 8)


def aimed(origins, targets, tmin=0.0, tmax=np.inf):
    """rays from float32 origins through float32 targets: d = fl(target - origin)"""
    o, p = f32(origins), f32(targets)
    o, p = np.broadcast_arrays(o, p)
    return rays_of(o, (p - o).astype(np.float32), tmin, tmax)


def _unit(rng, n):
    p = rng.normal(size=(n, 3))
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def surface_targets(vertices, faces, n, seed, min_weight=1.0 / 64):
    """(points float32 [n,3], face [n], outward-ish normal [n,3]) on random valid faces, every barycentric weight >= min_weight"""
    rng = np.random.default_rng(seed)
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    face = rng.integers(0, len(f), n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n) * (1 - 3 * 2 * min_weight) + 2 * min_weight
    tri = v[f[face]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return f32((w[:, :, None] * tri).sum(axis=1)), face, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


# ---------------------------------------------------------------- the cases
# a case: {"name", "vertices", "faces", "rays", "cell_cap" (None: the default), and what the case promises about the float32
# restatement, which tests/test_raycast_host.py checks: "hits" (per ray 1: hit, 0: miss, -1: no promise; or None), "all_hit" (every ray), "interior" (a mask of
# rays aimed at a point whose weights are all >= 1/64 of the nearest face, with "interior_face"), "winner" (face per ray, or None)}

def _case(name, mesh, rays, cell_cap=None, **promises):
    v, f = mesh
    case = {"name": name, "vertices": f32(v), "faces": np.ascontiguousarray(f, np.int32), "rays": np.ascontiguousarray(rays, np.float32),
            "cell_cap": cell_cap, "hits": None, "all_hit": False, "interior": None, "interior_face": None, "winner": None}
    case.update(promises)
    return case


def one_triangle_case():
    mesh = mc.one_triangle()                                 # (0,0,0), (1,0,0), (0,1,0)
    rays, hits = [], []
    add = lambda r, h: (rays.append(r), hits.extend([h] * len(r)))
    inner = [[0.25, 0.25, 0], [0.125, 0.5, 0], [0.5, 0.125, 0], [0.3125, 0.3125, 0]]
    rim = [[0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0, 0], [0, 0.75, 0], [0.25, 0.75, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]]
    for pts in (inner, rim):                                  # every coordinate exactly representable: on the rim the float64 fallback runs
        p = np.array(pts, np.float64)
        add(rays_of(p + [0, 0, 1], [0, 0, -1]), True)                        # straight down
        add(rays_of(p + [0, 0, -2], [0, 0, 2]), True)                        # from below: no culling
        add(rays_of(p + [0.5, -0.25, 2], [-0.5, 0.25, -2]), True)            # oblique, d exact
        add(rays_of(p + [-4, 2, 1], [4, -2, -1]), True)                      # kz = x
    add(rays_of([[-1, 0.25, 0], [0.25, -1, 0]], [[1, 0, 0], [0, 1, 0]]), False)              # in the triangle's plane
    add(rays_of([[0.25, 0.25, 0]], [[0, 0, 1]], tmin=0.0), True)                              # starts on the plane: t = 0
    add(rays_of([[0.25, 0.25, 1]], [[0, 0, -1]], tmax=1.0), True)                             # t == tmax
    add(rays_of([[0.25, 0.25, 1]], [[0, 0, -1]], tmax=np.nextafter(np.float32(1), np.float32(0))), False)
    add(rays_of([[0.25, 0.25, 1]], [[0, 0, -1]], tmin=np.nextafter(np.float32(1), np.float32(2))), False)
    add(rays_of([[2, 2, 1], [-0.5, 0.25, 1], [0.75, 0.75, 1]], [0, 0, -1]), False)            # beside it
    add(rays_of([[0.25, 0.25, 1]], [[0, 0, 1]]), False)                                       # behind the origin
    return _case("one_triangle", mesh, np.concatenate(rays), hits=np.array(hits).astype(np.int8))


def shared_edge_case(n=4096, seed=11):
    v = f32([[0.1, 0.2, 0.3], [1.3, 0.1, 0.5], [1.2, 1.4, 0.2], [0.05, 1.1, 0.7]])
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    rng = np.random.default_rng(seed)
    a, c = v[0].astype(np.float64), v[2].astype(np.float64)
    p = f32(a + rng.uniform(0.02, 0.98, (n, 1)) * (c - a))                  # float32-rounded points along the shared edge
    nrm = np.cross(v[1].astype(np.float64) - a, c - a)
    nrm /= np.linalg.norm(nrm)
    side = np.where(rng.random((n, 1)) < 0.5, 1.0, -1.0)
    o = p + side * nrm * rng.uniform(1.0, 3.0, (n, 1)) + rng.uniform(-0.4, 0.4, (n, 3))   # well off the plane on either side
    return _case("shared_edge", (v, f), aimed(o, p), all_hit=True)


def fan_case(n=512, seed=12):
    ring = [[np.cos(k * np.pi / 3), np.sin(k * np.pi / 3), 0.0] for k in range(6)]
    v = f32(np.array([[0.0, 0.0, 0.15]] + ring) * 0.7 + [0.3, 0.2, 0.1])   # a shallow cone around vertex 0
    f = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.int32)
    rng = np.random.default_rng(seed)
    side = np.where(rng.random((n, 1)) < 0.5, 1.0, -1.0)
    o = v[0] + side * np.array([0, 0, 1.0]) * rng.uniform(1.0, 4.0, (n, 1)) + np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), np.zeros((n, 1))], axis=1)
    return _case("fan", (v, f), aimed(o, v[0][None]), all_hit=True)


def icosphere_case(seed=13):
    mesh = mc.icosphere(3)                                   # 1 280 faces, radius 1
    rng = np.random.default_rng(seed)
    rays = []
    n_in = 768
    rays.append(aimed(3.0 * _unit(rng, n_in), 0.5 * _unit(rng, n_in) * rng.random((n_in, 1))))      # from outside at interior points
    rays.append(rays_of(0.3 * _unit(rng, 512) * rng.random((512, 1)), _unit(rng, 512)))             # from near the centre outwards
    n_all = n_in + 512
    pts, face, nrm = surface_targets(*mesh, 512, seed + 1)
    rays.append(aimed(pts + 2.0 * nrm + 0.2 * _unit(rng, 512), pts))                                # at points well inside a face
    o = 3.0 * _unit(rng, 256)
    rays.append(rays_of(o, np.cross(o, _unit(rng, 256)) + 0.2 * o))                                 # pass the box by
    corner = np.array([0.97, 0.97, 0.97]) * np.where(rng.random((256, 3)) < 0.5, 1.0, -1.0)
    rays.append(rays_of(corner, _unit(rng, 256)))                                                   # start inside the box, outside the sphere
    rays.append(rays_of(0.9 * _unit(rng, 256) * rng.random((256, 1)), _unit(rng, 256), tmin=0.0, tmax=rng.uniform(0.1, 3.0, 256)))
    rays = np.concatenate(rays)
    hits = np.full(len(rays), -1, np.int8)                   # -1: no promise
    hits[:n_all + 512] = 1
    interior = np.zeros(len(rays), bool)
    interior[n_all:n_all + 512] = True
    return _case("icosphere", mesh, rays, hits=hits, interior=interior, interior_face=face)


def cube_case():
    """an axis-aligned cube [-1, 1]^3; with cell_cap 64 its grid is 4 x 4 x 4 cells of edge 1/2: every cell boundary representable"""
    mesh = mc.cube_mesh()
    s = [-1.0, -0.5, 0.0, 0.25, 0.5, 1.0]                     # cube faces and edges, cell boundaries, a cell's inside
    rays = []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for a in s:
            for b in s:
                o = np.zeros(3)
                o[axis], o[u], o[w] = -3.0, a, b
                for d_u, d_w in ((0, 0), (0, 0.25), (0.125, 0), (0, -0.25)):           # two zero components, then one
                    d = np.zeros(3)
                    d[axis], d[u], d[w] = 1.0, d_u, d_w
                    rays += [rays_of(o[None], d[None]), rays_of(-o[None], -d[None])]
    for a in s:                                               # diagonals in the planes x = y and x = -y, at heights on and off boundaries
        rays += [rays_of([[-3.0, -3.0, a]], [[1.0, 1.0, 0.0]]), rays_of([[3.0, -3.0, a]], [[-1.0, 1.0, 0.0]]),
                 rays_of([[-2.0, -2.0, -2.0 + a]], [[1.0, 1.0, 1.0]])]
    rays += [rays_of([[0.25, 0.25, 0.25], [0.0, 0.0, 0.0], [0.5, 0.5, 0.5]], d[None]) for d in np.eye(3)]       # from inside
    return _case("cube", mesh, np.concatenate(rays), cell_cap=64)


def hygiene_case(seed=14):
    """degenerate faces, an index out of range, a NaN vertex, a face listed twice, two coincident faces under other indices"""
    v, f = mc.degenerate_mix()                                # 20 faces + collinear (20) + a point (21) + face 3 again (22)
    nv = len(v)
    v = np.concatenate([v, v[f[5]], [[np.nan, 0, 0]]]).astype(np.float32)             # copies of face 5's vertices: nv .. nv + 2; a NaN vertex
    f = np.concatenate([f, [[nv, nv + 1, nv + 2]], [[0, 1, nv + 40]], [[0, 1, nv + 3]], [[-1, 2, 3]], [[nv + 1, nv + 2, nv]]]).astype(np.int32)
    rng = np.random.default_rng(seed)
    rays = [aimed(3.0 * _unit(rng, 384), 0.4 * _unit(rng, 384)), rays_of(0.2 * _unit(rng, 128), _unit(rng, 128))]
    for face in (3, 5):                                       # straight at the doubled faces
        c = v[f[face]].astype(np.float64).mean(axis=0)
        rays.append(aimed(2.5 * c + 0.05 * _unit(rng, 32), c[None]))
    rays = np.concatenate(rays)
    return _case("hygiene", (v, f), rays)


def flat_case(seed=15):
    mesh = mc.plane_mesh()                                    # z = 0: one grid axis has a single cell
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-0.1, 1.0, (384, 1)), rng.uniform(-0.1, 0.8, (384, 1)), np.zeros((384, 1))], axis=1)
    o = p + np.concatenate([rng.uniform(-1, 1, (384, 2)), np.where(rng.random((384, 1)) < 0.5, 1.0, -1.0) * rng.uniform(0.05, 2.0, (384, 1))], axis=1)
    rays = [aimed(o, p), rays_of([[-0.5, 0.3, 0.0], [0.3, -0.5, 0.0], [-0.2, -0.2, 0.0]], [[1, 0, 0], [0, 1, 0], [1, 1, 0]])]
    return _case("flat", mesh, np.concatenate(rays))


def strip_mesh(n=128, length=100.0, width=0.05):
    """a long strip of 2 n faces in the plane z = 0"""
    x = np.linspace(0.0, length, n + 1)
    v = np.concatenate([np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1), np.stack([x, np.full_like(x, width), np.zeros_like(x)], axis=1)])
    f = [[i, i + 1, n + 2 + i] for i in range(n)] + [[i, n + 2 + i, n + 1 + i] for i in range(n)]
    return f32(v), np.array(f, np.int32)


def forced_grid_cases(seed=16):
    rng = np.random.default_rng(seed)
    out = []
    mesh = mc.icosphere(2)
    rays = np.concatenate([aimed(3.0 * _unit(rng, 256), 0.6 * _unit(rng, 256)), rays_of(3.0 * _unit(rng, 64), _unit(rng, 64))])
    out.append(_case("one_cell", mesh, rays, cell_cap=1))
    mesh = strip_mesh()                                       # cell_cap 2^20 over 100 x 0.05 x 0: the x axis hits the 1 024-cell cap, a face spans 8 cells
    p = np.stack([rng.uniform(-1, 101, 512), rng.uniform(-0.01, 0.06, 512), np.zeros(512)], axis=1)
    o = p + np.stack([rng.uniform(-3, 3, 512), rng.uniform(-0.5, 0.5, 512), rng.choice([-1.0, 1.0], 512) * rng.uniform(0.01, 2.0, 512)], axis=1)
    along = rays_of([[-1.0, 0.025, 0.001], [101.0, 0.0125, -0.002], [-1.0, 0.0, 0.0]], [[1.0, 0.0, -1e-5], [-1.0, 1e-4, 2e-5], [1.0, 0.0, 0.0]])
    out.append(_case("axis_cap", mesh, np.concatenate([aimed(o, p), along]), cell_cap=1 << 20))
    mesh = mc.stress_mesh(600)                                # one face across the whole box: the span margin at its largest
    p = mesh[0][mesh[1][rng.integers(1, len(mesh[1]), 512)]].astype(np.float64).mean(axis=1)     # centres of the small faces
    out.append(_case("stress", mesh, np.concatenate([aimed(p + 2.0 * _unit(rng, 512), p), rays_of(rng.uniform(0, 1, (128, 3)), _unit(rng, 128))])))
    return out


def invalid_rays():
    """rays the call answers with NaN, then a few legal ones with infinite bounds"""
    nan, inf = np.nan, np.inf
    bad = [[nan, 0, 3, 0, 0, -1, 0, inf], [0, inf, 3, 0, 0, -1, 0, inf], [0, 0, 3, 0, nan, -1, 0, inf], [0, 0, 3, -inf, 0, -1, 0, inf],
           [0, 0, 3, 0, 0, 0, 0, inf], [0, 0, 3, 0, 0, -0.0, 0, inf], [0, 0, 3, 0, 0, -1, nan, inf], [0, 0, 3, 0, 0, -1, 0, nan],
           [0, 0, 3, 0, 0, -1, 5, 1], [0, 0, 3, 0, 0, -1, inf, 0]]
    good = [[0, 0, 3, 0, 0, -1, -inf, inf], [0, 0, 3, 0, 0, -1, -inf, 2.5], [0, 0, 3, 0, 0, -1, inf, inf], [0, 0, 3, 0, 0, -1, -inf, -inf],
            [0, 0, 3, 0, 0, -1, 2, 2], [0, 0, 3, 0, 0, 1e-30, 0, inf], [0, 0, 3, 0, 0, -1e30, 0, inf]]
    return f32(bad), f32(good)


def ray_hygiene_case():
    bad, good = invalid_rays()
    return _case("ray_hygiene", mc.icosphere(1), np.concatenate([bad, good]), n_bad=len(bad))


@functools.lru_cache(maxsize=None)
def cases():
    return tuple([one_triangle_case(), shared_edge_case(), fan_case(), icosphere_case(), cube_case(), hygiene_case(), flat_case(),
                  ray_hygiene_case()] + forced_grid_cases())


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float32 and float64 restatements' results of a case, computed once: {"t32", "face32", "bary32", "hits32", "t64", "face64"}"""
    case = next(c for c in cases() if c["name"] == name)
    t32, f32_, b32, h32 = closest_hit(case["rays"], case["vertices"], case["faces"], np.float32)
    t64, f64, _, _ = closest_hit(case["rays"], case["vertices"], case["faces"], np.float64)
    return {"t32": t32, "face32": f32_, "bary32": b32, "hits32": h32, "t64": t64, "face64": f64}


def deviation(name):
    """the float32 restatement's own deviation from the float64 one over the rays both hit: max |t32 - t64|"""
    ref = reference(name)
    both = np.isfinite(ref["t32"]) & np.isfinite(ref["t64"])
    return float(np.abs(ref["t32"][both].astype(np.float64) - ref["t64"][both]).max()) if both.any() else 0.0
