"""Cases and the numpy restatement for the view-texturing tests (gpnerf_texture.hip; include/gpnerf_hip.h states THE DEFINITION restated
here, rule for rule, gpnerf_texture_points).

`restate(...)` is the definition in float64, vectorised over the points, one view at a time in ascending order: what the kernels must
give bit for bit.  Its rule 5 is THE INTERSECTION restated in float32 (raycast_cases.closest_hit over every face): the kernels' own
arithmetic there.  `restate(..., dtype=np.float32)` is the float32-projection variant: the projection and the bilinear sample carried out
in float32, the form the per-ray path's gather has -- its deviation from the float64 form is the yardstick of the convention
cross-check (4 x, the project's rule of DESIGN 4.18).  Nothing here looks at what the kernels give.
"""
import functools

import numpy as np

import mesh_metric_cases as mc
import raycast_cases as rc
from mesh_metric_cases import f32

USED, BEHIND, OUTSIDE, MASKED, BACKFACING, OCCLUDED = range(6)
FATES = ("used", "behind", "outside", "masked", "backfacing", "occluded")


def eyes_of(RTs):
    """-R^T T per view: float64, e_a = -((R[0][a] T0 + R[1][a] T1) + R[2][a] T2), rounded to float32"""
    RTs = np.asarray(RTs, np.float64).reshape(-1, 3, 4)
    return np.stack([[-((RT[0, a] * RT[0, 3] + RT[1, a] * RT[1, 3]) + RT[2, a] * RT[2, 3]) for a in range(3)] for RT in RTs]).astype(np.float32)


def project(points, K, RT, dtype=np.float64):
    """gpnerf_mesh_rasterize's projection of a vertex: (x, y, z) in dtype"""
    p = np.asarray(points, np.float32).astype(dtype)
    K, RT = np.asarray(K, np.float64).astype(dtype), np.asarray(RT, np.float64).astype(dtype)
    with np.errstate(all="ignore"):
        c = [((p[:, 0] * RT[r, 0] + p[:, 1] * RT[r, 1]) + p[:, 2] * RT[r, 2]) + RT[r, 3] for r in range(3)]
        h = [(c[0] * K[r, 0] + c[1] * K[r, 1]) + c[2] * K[r, 2] for r in range(3)]
        return h[0] / h[2], h[1] / h[2], h[2]


def bilinear(image, x, y, dtype=np.float64):
    """rule 6 at inside positions: image [H,W,C] float32, x, y [m] -> [m,C] in dtype"""
    H, W = image.shape[:2]
    x, y = x.astype(dtype), y.astype(dtype)
    fi, fj = np.floor(x), np.floor(y)
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
    fx, fy = (x - fi)[:, None], (y - fj)[:, None]
    img = image.astype(dtype)
    one = dtype(1)
    top = img[j0, i0] * (one - fx) + img[j0, i1] * fx
    bottom = img[j1, i0] * (one - fx) + img[j1, i1] * fx
    return top * (one - fy) + bottom * fy


def restate(points, Ks, RTs, images, normals=None, masks=None, vertices=None, faces=None, mode="blend", sharpness=2, cos_min=0.2,
            eps=1e-4, z_near=1e-6, fallback=None, background=0.0, dtype=np.float64):
    """THE DEFINITION -> {"color" float32 [n,C], "weight" float32 [n], "views" uint8 [n], "stats" int64 [V,6], "totals" int64 [2],
    "fate" [n,V], "w" float64 [n,V], "rows" float32 [n,V,8] (rule 5's rays), "xy" [n,V,2] in dtype}"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    Ks, RTs = np.asarray(Ks, np.float64).reshape(-1, 3, 3), np.asarray(RTs, np.float64).reshape(-1, 3, 4)
    images = np.asarray(images, np.float32)
    V, H, W, C = images.shape
    n = len(p)
    eyes = eyes_of(RTs)
    fate = np.full((n, V), USED, np.int64)
    w = np.zeros((n, V), np.float64)
    xy = np.zeros((n, V, 2), dtype)
    rows = np.zeros((n, V, 8), np.float32)
    rows[..., 5] = rows[..., 6] = 1.0                            # a decided pair: (0, 0, 0; 0, 0, 1; 1, 0), not a ray
    cos2 = float(cos_min) * float(cos_min)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        for v in range(V):
            x, y, z = project(p, Ks[v], RTs[v], dtype)
            xy[:, v, 0], xy[:, v, 1] = x, y
            open_ = np.ones(n, bool)

            def rule(name, keep):
                fate[open_ & ~keep, v] = name
                return open_ & keep

            open_ = rule(BEHIND, np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z >= dtype(z_near)))
            open_ = rule(OUTSIDE, (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1))
            if masks is not None:
                ok = np.zeros(n, bool)
                ok[open_] = np.asarray(masks)[v][np.rint(y[open_]).astype(np.int64), np.rint(x[open_]).astype(np.int64)] == 1
                open_ = rule(MASKED, ok)
            d = eyes[v][None, :] - p                             # float32
            if nrm is not None:
                d64 = d.astype(np.float64)
                a = (nrm[:, 0] * d64[:, 0] + nrm[:, 1] * d64[:, 1]) + nrm[:, 2] * d64[:, 2]
                nn = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
                vv = (d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2]
                open_ = rule(BACKFACING, (nn < np.inf) & (a > 0) & (a * a >= (cos2 * nn) * vv))
                r = (a * a) / (nn * vv)
                wv = np.ones(n) if sharpness == 0 else r.copy()
                for _ in range(1, sharpness):
                    wv = wv * r
                w[open_, v] = wv[open_]
            else:
                w[open_, v] = 1.0
            rows[open_, v, 0:3] = p[open_]
            rows[open_, v, 3:6] = d[open_]
            rows[open_, v, 6], rows[open_, v, 7] = np.float32(eps), 1.0
    if faces is not None and len(faces):
        # the nearest hit's t: +inf for a free segment (the ANY ray's t > 0), finite where a face lies between, NaN for a row that is no ray
        t = rc.closest_hit(rows.reshape(-1, 8), vertices, faces, np.float32)[0].reshape(n, V)
        fate[(fate == USED) & ~np.isposinf(t)] = OCCLUDED
    used = fate == USED
    colour = np.zeros((n, V, C), np.float64)
    for v in range(V):
        m = used[:, v]
        if m.any():
            colour[m, v] = bilinear(images[v], xy[m, v, 0], xy[m, v, 1], dtype).astype(np.float64)
    bg = np.broadcast_to(np.asarray(background, np.float32), (C,))
    out = np.empty((n, C), np.float32)
    out[:] = bg if fallback is None else np.asarray(fallback, np.float32).reshape(n, C)
    weight, views = np.zeros(n, np.float32), np.zeros(n, np.uint8)
    any_used = used.any(axis=1)
    with np.errstate(all="ignore"):
        if mode == "blend":
            S, D = np.zeros((n, C)), np.zeros(n)
            for v in range(V):
                m = used[:, v]
                S[m] = S[m] + w[m, v, None] * colour[m, v]
                D[m] = D[m] + w[m, v]
                views[m] |= np.uint8(1 << v)
            out[any_used] = (S[any_used] / D[any_used, None]).astype(np.float32)
            weight[any_used] = D[any_used].astype(np.float32)
        else:
            best, best_w = np.full(n, -1), np.zeros(n)
            for v in range(V):
                m = used[:, v] & ((best < 0) | (w[:, v] > best_w))
                best[m], best_w[m] = v, w[m, v]
            i = np.flatnonzero(any_used)
            out[i] = colour[i, best[i]].astype(np.float32)
            weight[i] = best_w[i].astype(np.float32)
            views[i] = (1 << best[i]).astype(np.uint8)
    stats = np.stack([[int((fate[:, v] == k).sum()) for k in range(6)] for v in range(V)]).astype(np.int64)
    totals = np.array([int(any_used.sum()), int((~any_used).sum())], np.int64)
    return {"color": out, "weight": weight, "views": views, "stats": stats, "totals": totals, "fate": fate, "w": w, "rows": rows, "xy": xy}


# ---------------------------------------------------------------- cases

def ring_cameras(n, H, W, focal=None, distance=3.0, target=(0.0, 0.0, 0.0), tilt=0.35):
    """n look_at cameras on a tilted ring around `target`"""
    focal = focal if focal is not None else 0.9 * min(H, W)
    Ks, RTs = [], []
    for k in range(n):
        a = 2 * np.pi * k / n + 0.3
        eye = np.asarray(target) + distance * np.array([np.cos(a) * np.cos(tilt), np.sin(a) * np.cos(tilt), np.sin(tilt) * (1 if k % 2 else -1)])
        K, RT = rc.look_at(eye, target, H, W, focal)
        Ks.append(K)
        RTs.append(RT)
    return np.stack(Ks), np.stack(RTs)


def axis_cameras(H=48, W=48, focal=60.0, distance=3.0):
    """the six look_at cameras of the sphere case: on +x, -x, +y, -y, +z, -z"""
    eyes = [[distance, 0, 0], [-distance, 0, 0], [0, distance, 0], [0, -distance, 0], [0, 0, distance], [0, 0, -distance]]
    pairs = [rc.look_at(e, [0, 0, 0], H, W, focal) for e in eyes]
    return np.stack([k for k, _ in pairs]), np.stack([r for _, r in pairs])


def random_images(V, H, W, C, seed):
    return np.random.default_rng(seed).random((V, H, W, C), dtype=np.float32)


def affine_image(H, W, coeffs):
    """[H,W,C] float64 with channel c = coeffs[c] . (column, row, 1)"""
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([a * col + b * row + c for a, b, c in coeffs], axis=-1)


def back_project(K, RT, x, y, z):
    """the float64 points that project to pixel (x, y) at camera depth z"""
    K, RT = np.asarray(K, np.float64), np.asarray(RT, np.float64)
    cam = np.linalg.solve(K, np.stack([x * z, y * z, z]))
    return (RT[:, :3].T @ (cam - RT[:, 3:4])).T


def special_points(K, RT, H, W, z_near):
    """points that are not points, and points exactly on the image's frame, for the camera (K, RT): float32 [m,3].  The frame points
    are found by stepping float32 candidates: what matters is that SOME land exactly on x = 0, x = W - 1 and y = H - 1."""
    z = 2.0
    frame = back_project(K, RT, np.array([0.0, W - 1.0, 0.5 * (W - 1), 0.0, W - 1.0]), np.array([0.5 * (H - 1), 0.5 * (H - 1), H - 1.0, 0.0, H - 1.0]),
                         np.full(5, z))
    eye = -RT[:, :3].T @ RT[:, 3]
    axis = RT[2, :3]
    behind = eye - 1.5 * axis
    at_near = eye + z_near * axis
    pts = [*frame, behind, at_near, eye, [np.nan, 0, 0], [0, np.inf, 0], [-np.inf, 0, 0], [1e30, -1e30, 1e30], [3e38, 3e38, 3e38]]
    return f32(np.asarray(pts, np.float64))


@functools.lru_cache(maxsize=None)
def general_case(n=65, V=8, H=20, W=24, C=3, seed=0, z_near=0.5):
    """n points in front of and around V ring cameras with an occluder (the unit icosphere, level 1) in the middle; normals of every
    kind; masks with 0, 1 and 100; the special points lead the list when n allows"""
    rng = np.random.default_rng(100 + seed)
    Ks, RTs = ring_cameras(V, H, W, focal=0.45 * min(H, W), distance=3.0)
    special = special_points(Ks[0], RTs[0], H, W, z_near)
    pts = f32(rng.normal(size=(max(n, 1), 3)) * 1.3)
    on = mc.sphere_points(max(n, 1), 1.0, seed=seed)                        # some exactly on the occluder's sphere
    pts[::3] = on[::3]
    if n >= 2 * len(special):
        pts[:len(special)] = special
    pts = pts[:n]
    nrm = f32(0.3 * pts + rng.normal(size=pts.shape))           # loosely outward: some face a camera from behind the occluder
    if n >= 8:
        nrm[-1] = 0.0
        nrm[-2] = [np.nan, 1.0, 0.0]
        nrm[-3] = [np.inf, 0.0, 0.0]
        nrm[-4] = nrm[-4] * np.float32(1e-20)
        nrm[-5] = nrm[-5] * np.float32(1e18)
    images = random_images(V, H, W, C, seed)
    masks = rng.choice(np.array([0, 1, 1, 1, 1, 1, 1, 100], np.uint8), size=(V, H, W))
    v, f = mc.icosphere(1)
    fallback = f32(rng.random((n, C)))
    return {"points": pts, "normals": nrm, "Ks": Ks, "RTs": RTs, "images": images, "masks": masks, "vertices": v, "faces": f,
            "fallback": fallback, "z_near": z_near, "H": H, "W": W}


def exact_case():
    """A camera whose projection is exact (R = I, T = 0, K = (8, 0, 4; 0, 8, 4; 0, 0, 1), 9 x 9: z = p2, x = 8 p0 / p2 + 4 without a
    rounding at z = 1): points at z = z_near exactly, one ulp below (BEHIND) and one above; points exactly on x = 0, x = W - 1, y = 0
    and y = H - 1 and the four corners (USED: the frame is inclusive), and one ulp beyond each side (OUTSIDE).  "expect" names each
    point's fate."""
    z_near = float(np.float32(0.75))
    K = np.array([[8.0, 0, 4.0], [0, 8.0, 4.0], [0, 0, 1.0]])
    RT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    below, above = np.nextafter(np.float32(z_near), np.float32(0)), np.nextafter(np.float32(z_near), np.float32(2))
    up = np.nextafter(np.float32(0.5), np.float32(1))
    pts = [[0, 0, z_near], [0, 0, below], [0, 0, above],
           [-0.5, 0, 1], [0.5, 0, 1], [0, -0.5, 1], [0, 0.5, 1], [-0.5, -0.5, 1], [0.5, -0.5, 1], [-0.5, 0.5, 1], [0.5, 0.5, 1],
           [-up, 0, 1], [up, 0, 1], [0, -up, 1], [0, up, 1]]
    expect = [USED, BEHIND, USED] + [USED] * 8 + [OUTSIDE] * 4
    return {"points": f32(pts), "Ks": K[None], "RTs": RT[None], "z_near": z_near, "H": 9, "W": 9, "expect": np.array(expect)}


@functools.lru_cache(maxsize=None)
def sphere_case():
    """icosphere(3): 642 vertices, radius 1, normals = positions; six axis cameras at distance 3, 48 x 48, focal 60"""
    v, f = mc.icosphere(3)
    Ks, RTs = axis_cameras()
    colours = f32(0.5 + 0.25 * v.astype(np.float64) @ np.array([[1.0, 0.2, -0.4], [-0.3, 1.0, 0.5], [0.4, -0.6, 1.0]]) / 1.5)
    return {"vertices": v, "faces": f, "normals": v.copy(), "Ks": Ks, "RTs": RTs, "H": 48, "W": 48, "colours": colours, "cos_min": 0.2}


def squares_case(H=128, W=128, focal=120.0):
    """A unit square at z = 0 facing +z (two faces) and a smaller one in front at z = 1 (half the side), one camera on the +z axis at
    z = 3; a lattice of points on the back square none of which projects within one pixel of the front square's outline or of the
    back square's own.  The colours are dyadic, so that a weighted mean of equal values rounds back to the value."""
    v = f32([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0],
             [-0.25, -0.25, 1], [0.25, -0.25, 1], [0.25, 0.25, 1], [-0.25, 0.25, 1]])
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    K, RT = rc.look_at([0, 0, 3.0], [0, 0, 0], H, W, focal)
    # the front square's outline projects to 0.25 focal / 2 = 15 pixels from the centre, the back square's to 0.5 focal / 3 = 20; a
    # back point (a, b, 0) projects to focal a / 3 = 40 a from it, and the segment to the eye crosses z = 1 at (2 a / 3, 2 b / 3): the
    # shadow's edge on the back square is |a| = 0.375.  Of the coordinates k / 32 the lattice keeps those more than one pixel from
    # both outlines: 40 | |a| - 0.375 | > 1 drops k = 12, and 40 |a| < 19 ends at k = 15
    g = np.arange(-15, 16) / 32.0
    g = g[(np.abs(np.abs(g) - 0.375) * focal / 3.0 > 1.0) & (np.abs(g) * focal / 3.0 < 0.5 * focal / 3.0 - 1.0)]
    a, b = np.meshgrid(g, g, indexing="ij")
    pts = f32(np.stack([a.ravel(), b.ravel(), np.zeros(a.size)], axis=1))
    shadowed = (np.abs(pts[:, 0]) < 0.375) & (np.abs(pts[:, 1]) < 0.375)
    colours = f32([[0.25, 0.5, 0.75]] * 4 + [[0.75, 0.25, 0.5]] * 4)
    return {"vertices": v, "faces": f, "K": K, "RT": RT, "H": H, "W": W, "points": pts, "shadowed": shadowed, "colours": colours,
            "back": colours[0], "front": colours[4], "focal": focal}
