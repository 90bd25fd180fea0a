"""The per-face texture atlas (gpnerf_atlas.hip) restated in numpy from the text of include/gpnerf_hip.h -- THE DEFINITION 1 (the
parameterisation and its packing), 2 (the texels' surface points), 4 (the pack) and 5 (the shade) -- and the cases of its tests.  The
bake has no restatement of its own: it is texture_cases.restate on the restated texel points.  float64, multiply then add in the order
written, rounded to float32 once: what the kernels must give bit for bit.  Nothing here looks at what the kernels give."""
import functools

import numpy as np

import mesh_metric_cases as mm
import raster_cases as ras
import texture_cases as tc
from mesh_metric_cases import f32

UNOWNED, SEEN, FALLBACK, GUTTER = range(4)
RES_MIN, RES_MAX, MAX_SIDE = 2, 64, 16384


# ---------------------------------------------------------------- 1. the parameterisation

def layout(n_faces, R):
    """{cells_x, cells_y, width, height, texels_per_face, n_texels, cells}, or None for what gpnerf_atlas_layout refuses"""
    if not (RES_MIN <= R <= RES_MAX) or n_faces < 0 or n_faces >= 2 ** 31:
        return None
    P = (n_faces + 1) // 2
    cx = 0
    while cx * cx < P:
        cx += 1
    cy = -(-P // cx) if cx else 0
    tpf = R * (R + 1) // 2
    lay = dict(cells_x=cx, cells_y=cy, width=cx * (R + 2), height=cy * R, texels_per_face=tpf, n_texels=n_faces * tpf, cells=P)
    if lay["width"] > MAX_SIDE or lay["height"] > MAX_SIDE or lay["n_texels"] >= 2 ** 31:
        return None
    return lay


def texel_ij(R):
    """(i [tpf], j [tpf]) in the order of the index t = j R - j (j - 1) / 2 + i"""
    ij = [(i, j) for j in range(R) for i in range(R - j)]
    i, j = np.array([a for a, _ in ij], np.int64), np.array([b for _, b in ij], np.int64)
    assert np.array_equal(j * R - j * (j - 1) // 2 + i, np.arange(R * (R + 1) // 2))
    return i, j


def texel_pixels(n_faces, R):
    """(X [n_faces, tpf], Y [n_faces, tpf]): the image position of every texel, by the packing"""
    lay = layout(n_faces, R)
    i, j = texel_ij(R)
    f = np.arange(n_faces, dtype=np.int64)[:, None]
    q, odd = f // 2, (f % 2) == 1
    x = np.where(odd, R + 1 - i[None], i[None])
    y = np.where(odd, R - 1 - j[None], j[None])
    cx = max(lay["cells_x"], 1)
    return (q % cx) * (R + 2) + x, (q // cx) * R + y


def owner(n_faces, R):
    """The packing inverted at every image texel -> (kind [Ht,Wt] in {UNOWNED, 1 = owned, GUTTER}, face, i, j [Ht,Wt], -1 where not owned)"""
    lay = layout(n_faces, R)
    Ht, Wt, cx, P = lay["height"], lay["width"], lay["cells_x"], lay["cells"]
    Y, X = np.meshgrid(np.arange(Ht, dtype=np.int64), np.arange(Wt, dtype=np.int64), indexing="ij")
    q = (Y // R) * cx + X // (R + 2)
    x, y = X % (R + 2), Y % R
    odd = x + y > R
    face = 2 * q + odd
    kind = np.ones((Ht, Wt), np.int64)
    kind[face >= n_faces] = UNOWNED
    kind[x + y == R] = GUTTER
    kind[q >= P] = UNOWNED
    own = kind == 1
    i, j = np.where(odd, R + 1 - x, x), np.where(odd, R - 1 - y, y)
    return kind, np.where(own, face, -1), np.where(own, i, -1), np.where(own, j, -1)


def face_uvs(n_faces, R):
    """float64 [n_faces,3,2]: (u, v) of the corner texels a, b, c"""
    lay = layout(n_faces, R)
    X, Y = texel_pixels(n_faces, R)
    i, j = texel_ij(R)
    corner = [int(np.flatnonzero((i == a) & (j == b))[0]) for a, b in ((0, 0), (R - 1, 0), (0, R - 1))]
    return np.stack([(X[:, corner] + 0.5) / max(lay["width"], 1), 1.0 - (Y[:, corner] + 0.5) / max(lay["height"], 1)], axis=-1)


# ---------------------------------------------------------------- 2. the texels' surface points

def _combine(wa, wb, wc, a, b, c):
    with np.errstate(all="ignore"):
        return ((wa[None, :, None] * a[:, None, :] + wb[None, :, None] * b[:, None, :]) + wc[None, :, None] * c[:, None, :]).astype(np.float32)


def texels(vertices, faces, R, normals=None, attrs=None, first_face=0, count=None):
    """-> {"points" [T,3], "normals" [T,3], "attrs" [T,C] (with attrs)} float32, the faces first_face .. first_face + count - 1"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    count = len(f) - first_face if count is None else count
    f = f[first_face:first_face + count]
    i, j = texel_ij(R)
    d = float(R - 1)
    wb, wc, wa = i.astype(np.float64) / d, j.astype(np.float64) / d, (R - 1 - i - j).astype(np.float64) / d
    bad = ((f < 0) | (f >= len(v))).any(axis=1)
    fs = np.where(bad[:, None], 0, f)
    v64 = v.astype(np.float64) if len(v) else np.zeros((1, 3))
    a, b, c = v64[fs[:, 0]], v64[fs[:, 1]], v64[fs[:, 2]]
    tpf = len(i)
    out = {"points": _combine(wa, wb, wc, a, b, c)}
    if normals is not None:
        n64 = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
        out["normals"] = _combine(wa, wb, wc, n64[fs[:, 0]], n64[fs[:, 1]], n64[fs[:, 2]])
    else:
        with np.errstate(all="ignore"):
            u, w = b - a, c - a
            fn = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]],
                          axis=1).astype(np.float32)
        out["normals"] = np.repeat(fn[:, None, :], tpf, axis=1)
    if attrs is not None:
        a64 = np.asarray(attrs, np.float32).reshape(len(v), -1).astype(np.float64)
        out["attrs"] = _combine(wa, wb, wc, a64[fs[:, 0]], a64[fs[:, 1]], a64[fs[:, 2]])
    for k in out:
        out[k] = out[k].copy()
        out[k][bad] = np.nan
        out[k] = np.ascontiguousarray(out[k].reshape(len(f) * tpf, -1))
    return out


# ---------------------------------------------------------------- 3. the bake

def bake(vertices, faces, R, Ks, RTs, images, normals=None, masks=None, fallback=None, **kw):
    """texture_cases.restate on the restated texel points, hidden by the mesh itself (brute force over every face); fallback per vertex"""
    t = texels(vertices, faces, R, normals=normals, attrs=fallback)
    return tc.restate(t["points"], Ks, RTs, images, normals=t["normals"], masks=masks, vertices=vertices, faces=faces,
                      fallback=t.get("attrs"), **kw), t


# ---------------------------------------------------------------- 4. the pack

def pack(colors, views, n_faces, R, background=0.0):
    """-> (image float32 [Ht,Wt,C], coverage uint8 [Ht,Wt])"""
    lay = layout(n_faces, R)
    colors = np.asarray(colors, np.float32).reshape(lay["n_texels"], -1)
    C = colors.shape[1]
    bg = np.broadcast_to(np.asarray(background, np.float32), (C,))
    kind, face, i, j = owner(n_faces, R)
    Ht, Wt = kind.shape
    row = np.where(kind == 1, face * lay["texels_per_face"] + j * R - j * (j - 1) // 2 + i, 0)
    image = np.empty((Ht, Wt, C), np.float32)
    image[:] = bg
    own = kind == 1
    image[own] = colors[row[own]]
    coverage = np.zeros((Ht, Wt), np.uint8)
    seen = np.ones(lay["n_texels"], bool) if views is None else np.asarray(views).reshape(-1) != 0
    coverage[own] = np.where(seen[row[own]], SEEN, FALLBACK)
    coverage[kind == GUTTER] = GUTTER
    for Y, X in zip(*np.nonzero(kind == GUTTER)):
        total, n = np.zeros(C, np.float64), 0
        for nx, ny in ((X - 1, Y), (X, Y - 1), (X + 1, Y), (X, Y + 1)):            # left, upper, right, lower
            if 0 <= nx < Wt and 0 <= ny < Ht and kind[ny, nx] == 1:
                with np.errstate(all="ignore"):
                    total = total + colors[row[ny, nx]].astype(np.float64)
                n += 1
        if n:
            with np.errstate(all="ignore"):
                image[Y, X] = (total / float(n)).astype(np.float32)
    return image, coverage


# ---------------------------------------------------------------- 5. the shade

def shade(face_id, vertices, faces, cams, H, W, image, R, filter="simplex", background=0.0, z_near=ras.Z_NEAR):
    """gpnerf_atlas_shade restated -> (float32 [V,H,W,C], shaded bool [V,H,W]).  The covered pixels and their ub, uc are
    raster_cases.interpolate_np's, restated there from gpnerf_mesh_interpolate."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    image = np.asarray(image, np.float32)
    C = image.shape[2]
    cams = np.asarray(cams, np.float64).reshape(-1, 21)
    lay = layout(len(fc), R)
    cxn = max(lay["cells_x"], 1)
    out = np.empty((len(cams), H * W, C), np.float32)
    out[:] = np.broadcast_to(np.asarray(background, np.float32), (C,))
    shaded = np.zeros((len(cams), H * W), bool)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    px, py = 256 * ii.reshape(-1), 256 * jj.reshape(-1)
    top = float(R - 1)
    for w in range(len(cams)):
        x, y, z = ras.project(v, cams[w])
        usable, X, Y = ras.snap(x, y, z, z_near)
        fs, bad, flat, A = ras.face_states(fc, len(v), usable, X, Y)
        fid = np.asarray(face_id)[w].reshape(-1).astype(np.int64)
        pi = np.nonzero((fid >= 0) & (fid < len(fs)))[0]
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
        f = fid[pi]
        with np.errstate(all="ignore"):
            Ad = area.astype(np.float64)
            ta, tb, tcc = (ea.astype(np.float64) / Ad) / z[a], (eb.astype(np.float64) / Ad) / z[b], (ec.astype(np.float64) / Ad) / z[c]
            q = (ta + tb) + tcc
            ub, uc = tb / q, tcc / q
            s = ub * top
            s = np.where(s > 0.0, s, 0.0)
            s = np.where(s < top, s, top)
            room = top - s
            t = uc * top
            t = np.where(t > 0.0, t, 0.0)
            t = np.where(t < room, t, room)
        i0 = np.minimum(np.floor(s).astype(np.int64), R - 1)
        j0 = np.minimum(np.floor(t).astype(np.int64), R - 1 - i0)
        fs_, ft = s - i0, t - j0
        lower = (fs_ + ft <= 1.0) | (i0 + j0 >= R - 2)
        wts = [(1.0 - fs_) - ft, np.where(lower, fs_, 1.0 - ft), np.where(lower, ft, 1.0 - fs_), (fs_ + ft) - 1.0]
        is_tap = [lower, np.ones(len(pi), bool), np.ones(len(pi), bool), ~lower]
        S, D = np.zeros((len(pi), C)), np.zeros(len(pi))
        best_w, best_c, have = np.zeros(len(pi)), np.zeros((len(pi), C), np.float32), np.zeros(len(pi), bool)
        odd = (f % 2) == 1
        cell = f // 2
        for k in range(4):
            i, j = i0 + (k & 1), j0 + (k >> 1)
            read = is_tap[k] & (i + j <= R - 1)
            xx, yy = np.where(odd, R + 1 - i, i), np.where(odd, R - 1 - j, j)
            IX, IY = (cell % cxn) * (R + 2) + xx, (cell // cxn) * R + yy
            col = np.zeros((len(pi), C), np.float32)
            col[read] = image[IY[read], IX[read]]                                   # a tap that is not read is not indexed
            with np.errstate(all="ignore"):
                S[read] = S[read] + wts[k][read, None] * col[read].astype(np.float64)
                D[read] = D[read] + wts[k][read]
            take = read & (~have | (wts[k] > best_w))
            best_w[take], best_c[take] = wts[k][take], col[take]
            have |= read
        with np.errstate(all="ignore"):
            out[w, pi] = (S / D[:, None]).astype(np.float32) if filter == "simplex" else best_c
        shaded[w, pi] = True
    return out.reshape(len(cams), H, W, C), shaded.reshape(len(cams), H, W)


# ---------------------------------------------------------------- cases

def random_mesh(n_faces, seed=0):
    """n_faces faces cut from an icosphere large enough (shared edges and an odd count where n_faces is odd)"""
    level = 0
    while 20 * 4 ** level < n_faces:
        level += 1
    v, f = mm.icosphere(level)
    return v, np.ascontiguousarray(f[:n_faces], np.int32)


def analytic_colour(p):
    """0.5 + 0.4 sin(6 p / |p| + (1, -2, 0)): [n,3] float64 -> [n,3]"""
    p = np.asarray(p, np.float64)
    return 0.5 + 0.4 * np.sin(6.0 * p / np.linalg.norm(p, axis=1, keepdims=True) + np.array([1.0, -2.0, 0.0]))


def surface_pictures(vertices, faces, cams, H, W, fid):
    """The pictures of the analytic case: at every covered pixel the analytic colour at the pixel's surface point (perspective-correct
    weights of the winning face) -> float32 [V,H,W,3]; 0 elsewhere"""
    pos = ras.interpolate_np(fid, vertices, faces, cams, H, W, np.asarray(vertices, np.float32), 0.0).astype(np.float64)
    img = np.zeros(pos.shape, np.float32)
    covered = fid >= 0
    img[covered] = analytic_colour(pos[covered]).astype(np.float32)
    return img


def area_weighted_normals(vertices, faces):
    v64, f = np.asarray(vertices, np.float32).astype(np.float64), np.asarray(faces, np.int64)
    fn = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    nrm = np.zeros_like(v64)
    for k in range(3):
        np.add.at(nrm, f[:, k], fn)
    return nrm.astype(np.float32)


@functools.lru_cache(maxsize=None)
def analytic_case(level=1, size=64):
    """The case of the test that fails without the feature: icosphere(level), size x size, the six axis cameras plus two of a ring of
    four as sources and the ring's other two held out, pictures of the analytic colour drawn from the SAME mesh, masks = coverage"""
    v, f = mm.icosphere(level)
    aK, aRT = tc.axis_cameras(size, size, focal=83.2 * size / 64)
    rK, rRT = tc.ring_cameras(4, size, size, focal=83.2 * size / 64, tilt=0.6)
    Ks, RTs = np.concatenate([aK, rK[:2], rK[2:]]), np.concatenate([aRT, rRT[:2], rRT[2:]])
    cams = np.concatenate([Ks.reshape(-1, 9), RTs.reshape(-1, 12)], axis=1)
    fid = ras.rasterize_np(v, f, cams, size, size)["face_id"]
    images = surface_pictures(v, f, cams, size, size, fid)
    masks = (fid >= 0).astype(np.uint8)
    case = dict(v=v, f=f, Ks=Ks, RTs=RTs, cams=cams, fid=fid, images=images, masks=masks, size=size, source=np.arange(8), held=np.arange(8, 10),
                vertex_normals=area_weighted_normals(v, f))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def psnr(image, truth, counted):
    d = (np.asarray(image, np.float32) - np.asarray(truth, np.float32))[counted].astype(np.float64)
    return -10.0 * np.log10((d * d).mean())


@functools.lru_cache(maxsize=None)
def analytic_reference(level=1, size=64):
    """The float64 restatement's held-out figures on analytic_case: {"vertex": dB, 4: dB, 8: dB, "seen": {...}, "images": {...}}"""
    c = analytic_case(level, size)
    s, h = c["source"], c["held"]
    v, f = c["v"], c["f"]
    counted = c["fid"][h] >= 0
    vert = tc.restate(v, c["Ks"][s], c["RTs"][s], c["images"][s], normals=c["vertex_normals"], masks=c["masks"][s], vertices=v, faces=f)
    drawn = ras.interpolate_np(c["fid"][h], v, f, c["cams"][h], size, size, vert["color"], 0.0)
    out = {"vertex": psnr(drawn, c["images"][h], counted), "images": {"vertex": drawn}, "counted": counted, "colors": {"vertex": vert["color"]}}
    corner_seen = vert["views"][f] != 0                            # [nf,3]: the colours the held-out pixels interpolate
    out["seen"] = {"vertex": bool(corner_seen[np.unique(c["fid"][h][counted])].all())}
    for R in (4, 8):
        b, _ = bake(v, f, R, c["Ks"][s], c["RTs"][s], c["images"][s], masks=c["masks"][s])
        image, coverage = pack(b["color"], b["views"], len(f), R)
        drawn, shaded = shade(c["fid"][h], v, f, c["cams"][h], size, size, image, R)
        out[R] = psnr(drawn, c["images"][h], counted)
        out["images"][R] = drawn
        out["colors"][R] = b["color"]
        tpf = R * (R + 1) // 2
        face_seen = (b["views"].reshape(len(f), tpf) != 0).all(axis=1)
        out["seen"][R] = bool(face_seen[np.unique(c["fid"][h][counted])].all()) and bool((shaded == counted).all())
    return out
