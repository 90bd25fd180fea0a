"""A mesh in calibrated cameras: drawing it, scoring its silhouettes, colouring it from the views and baking a texture atlas
(csrc/gpnerf_raster.hip, gpnerf_texture.hip, gpnerf_atlas.hip).

In: a device mesh (contiguous float32 vertices [n,3], int32 faces [m,3]; the rasteriser also takes a mesh.Mesh or a pair alone and
uploads it), host cameras Ks [v,3,3] and RTs [v,3,4] used in float64, and device images float32 [v,H,W,C] or masks uint8 [v,H,W].
Out, on the device: depth, face-id and attribute images (rasterize_mesh), silhouette counts (silhouette_stats), per-point or
per-vertex colours with their weights and view bits (texture_points, texture_mesh), a per-face TextureAtlas (texture_atlas and its
steps atlas_texels, atlas_pack; atlas_layout and atlas_face_uvs are host arithmetic).  The read_* functions name the counts on the
host.  frame re-exports every public name."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._args import _points, _raster_cams, _raster_mesh, _stream_ptr, _workspace, host_int64, mesh_args, ptr, row_dict, tensor_arg
from .mesh_query import MeshGrid, build_mesh_grid


def rasterize_mesh(vertices, faces, Ks, RTs, H, W, z_near=1e-6, want=("depth", "face_id"), attributes=None, background=0.0):
    """gpnerf_mesh_rasterize (and gpnerf_mesh_interpolate when `attributes` are given): the mesh drawn into the cameras Ks [n,3,3],
    RTs [n,3,4] (host arrays, used in float64; T in the vertices' unit: visual_hull's cameras) at H x W.  vertices, faces: device
    float32 [nv,3] and int32 [nf,3]; or faces=None and `vertices` a mesh.Mesh or a (vertices, faces) pair, which mesh_to_device uploads
    (host arrays go to cuda:0).  include/gpnerf_hip.h states what a pixel receives: the nearest face covering its centre, edges
    inclusive, the smaller face index among equal depths, bit-reproducible.
    Returns a dict of device tensors: "depth" float32 [n,H,W] (+inf where empty) and "face_id" int32 [n,H,W] (-1 there) as `want`
    names them, "stats" int64 [n,4] (_lib.RASTER_*: faces drawn, skipped for a vertex, skipped for zero area, pixels covered), and
    "image" float32 [n,H,W,C] when attributes -- device float32 [nv,C] or [nv], C <= 4, e.g. vertex colours or normals -- are given:
    interpolated perspective-correctly over the winning faces, `background` (a number or C numbers) elsewhere.  Nothing is read back."""
    lib = L.lib()
    vertices, faces = _raster_mesh(vertices, faces, "rasterize_mesh")
    unknown = set(want) - {"depth", "face_id"}
    if unknown:
        raise L.GpnerfError(f"rasterize_mesh: want names {sorted(unknown)}; depth and face_id are what there is")
    cams = _raster_cams(Ks, RTs, "rasterize_mesh")
    n, nv, nf, dev = cams.shape[0], int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    H, W = int(H), int(W)
    nbytes = int(lib.gpnerf_mesh_raster_workspace_bytes(nf, n, H, W))
    if nbytes <= 0:
        raise L.GpnerfError(f"rasterize_mesh: refused ({nf} faces, {n} views, {H} x {W})")
    ws = _workspace(dev, nbytes)
    res = {"stats": torch.empty((n, 4), device=dev, dtype=torch.int64)}
    if "depth" in want:
        res["depth"] = torch.empty((n, H, W), device=dev, dtype=torch.float32)
    face_id = torch.empty((n, H, W), device=dev, dtype=torch.int32) if "face_id" in want or attributes is not None else None
    if "face_id" in want:
        res["face_id"] = face_id
    L.check(lib.gpnerf_mesh_rasterize(ptr(vertices), nv, ptr(faces), nf, cams.ctypes.data_as(L.DP), n, H, W, float(z_near), ws.data_ptr(),
                                      ws.numel(), ptr(res.get("depth")), ptr(face_id), res["stats"].data_ptr(), _stream_ptr(dev)),
            "gpnerf_mesh_rasterize")
    if attributes is not None:
        attrs = attributes.reshape(nv, -1) if isinstance(attributes, torch.Tensor) and attributes.dim() == 1 else attributes
        tensor_arg(attrs, "rasterize_mesh: attributes", torch.float32, (nv, None), device=dev)
        c = int(attrs.shape[1])
        if not 1 <= c <= L.RASTER_MAX_ATTRS:
            raise L.GpnerfError(f"rasterize_mesh: 1 to {L.RASTER_MAX_ATTRS} attribute channels, got {c}")
        bg = np.broadcast_to(np.asarray(background, dtype=np.float32), (c,))
        res["image"] = torch.empty((n, H, W, c), device=dev, dtype=torch.float32)
        L.check(lib.gpnerf_mesh_interpolate(face_id.data_ptr(), ptr(vertices), nv, ptr(faces), nf, cams.ctypes.data_as(L.DP), n, H, W, float(z_near),
                                            ptr(attrs), c, (C.c_float * c)(*[float(b) for b in bg]), res["image"].data_ptr(), _stream_ptr(dev)),
                "gpnerf_mesh_interpolate")
    return res


def silhouette_stats(face_id, masks, out=None):
    """gpnerf_silhouette_stats: device int64 [n,5] (_lib.SILHOUETTE_*: covered, gt, both, either over the pixels whose mask is not the
    border band's 100, and the number of those left out) from rasterize_mesh's face_id int32 [n,H,W] and the views' masks, device
    uint8 [n,H,W] (0, 1, border 100).  out: a [n,5] int64 slot to write into.  Nothing is read back."""
    lib = L.lib()
    tensor_arg(face_id, "silhouette_stats: face_id", torch.int32, (None, None, None))
    tensor_arg(masks, "silhouette_stats: masks", torch.uint8, like=face_id, device=face_id.device)
    n, H, W = (int(s) for s in face_id.shape)
    if out is None:
        out = torch.empty((n, L.SILHOUETTE_COUNTS), device=face_id.device, dtype=torch.int64)
    L.check(lib.gpnerf_silhouette_stats(face_id.data_ptr(), masks.data_ptr(), n, H, W, out.data_ptr(), _stream_ptr(face_id.device)),
            "gpnerf_silhouette_stats")
    return out


def read_silhouette_metrics(host_counts):
    """silhouette_stats' counts on the host ([n,5], array or tensor) -> {"iou", "precision", "recall": the means over the views,
    "per_view": {"iou": [...], "precision": [...], "recall": [...], "ignored": [...]}}.  iou = both / either, precision = both / covered,
    recall = both / gt; 0 / 0 is 1.0 (nothing drawn where nothing is to be drawn is a match)."""
    c = host_int64(host_counts).reshape(-1, L.SILHOUETTE_COUNTS)
    if not len(c):
        raise L.GpnerfError("read_silhouette_metrics: no view")
    ratio = lambda num, den: [float(a) / float(b) if b else 1.0 for a, b in zip(c[:, num], c[:, den])]
    per = {"iou": ratio(L.SILHOUETTE_BOTH, L.SILHOUETTE_EITHER), "precision": ratio(L.SILHOUETTE_BOTH, L.SILHOUETTE_COVERED),
           "recall": ratio(L.SILHOUETTE_BOTH, L.SILHOUETTE_GT)}
    res = {k: float(np.mean(v)) for k, v in per.items()}
    per["ignored"] = [int(v) for v in c[:, L.SILHOUETTE_IGNORED]]
    res["per_view"] = per
    return res


TEXTURE_WANT = ("color", "weight", "views")


def face_vertex_normals(vertices, faces):
    """Area-weighted vertex normals of a device mesh -> float32 [n,3], not normalised: every face's cross product (b - a) x (c - a) in
    float64, added to its three vertices by index_add_ in face order.  A vertex no face names gets the zero vector."""
    nv, _ = mesh_args(vertices, faces, "face_vertex_normals", min_faces=1)
    v, f = vertices.to(torch.float64), faces.to(torch.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    fn = torch.cross(b - a, c - a, dim=1)
    out = torch.zeros((nv, 3), device=vertices.device, dtype=torch.float64)
    for k in range(3):
        out.index_add_(0, f[:, k], fn)
    return out.to(torch.float32).contiguous()


def texture_points(points, Ks, RTs, images, normals=None, masks=None, vertices=None, faces=None, grid=None, mode="blend", sharpness=2,
                   cos_min=0.2, eps=1e-4, z_near=1e-6, fallback=None, background=0.0, want=TEXTURE_WANT):
    """gpnerf_texture_points: the colour the views give each of the device float32 points [n,3].  Ks [m,3,3], RTs [m,3,4]: host arrays,
    used in float64, rasterize_mesh's cameras (1 to 8); images: device float32 [m,H,W,C], channels last, C <= 4 (Frame.imgs as it is).
    include/gpnerf_hip.h states what a point receives: per view it is left out when it is behind the camera, outside the image, off
    the mask (masks: device uint8 [m,H,W], 1 = foreground), facing away (normals: device float32 [n,3], any length; the cosine to the
    eye must reach cos_min) or hidden by the mesh (grid: a MeshGrid, or vertices and faces for the brute-force form; neither: no
    occlusion test; eps: mesh_visibility's); the views that remain are sampled bilinearly and blended with the weights cosine^(2
    sharpness) (mode "blend"), or the one of the largest weight is taken (mode "best").  A point no view sees gets its row of
    fallback (device float32 [n,C]) or background (a number or C numbers).
    Returns a dict of device tensors: "color" float32 [n,C], "weight" float32 [n] and "views" uint8 [n] (bit v: view v was used) as
    `want` names them, "stats" int64 [m,6] (_lib.TEXTURE_STATS: the points of each view under their fate) and "totals" int64 [2]
    (points some view saw, points none did).  Nothing is read back."""
    lib = L.lib()
    if mode not in L.TEXTURE_MODES:
        raise L.GpnerfError(f"texture_points: mode is 'blend' or 'best', got {mode!r}")
    unknown = set(want) - set(TEXTURE_WANT)
    if unknown:
        raise L.GpnerfError(f"texture_points: want names {sorted(unknown)}; color, weight and views are what there is")
    points = _points(points, "texture_points: points")
    dev, n = points.device, int(points.shape[0])
    cams = _raster_cams(Ks, RTs, "texture_points")
    m = cams.shape[0]
    tensor_arg(images, "texture_points: images", torch.float32, (m, None, None, None), device=dev)
    H, W, c = (int(s) for s in images.shape[1:])
    if not 1 <= c <= L.TEXTURE_MAX_CHANNELS:
        raise L.GpnerfError(f"texture_points: 1 to {L.TEXTURE_MAX_CHANNELS} channels, got {c}")
    if normals is not None:
        normals = _points(normals, "texture_points: normals", like=points, device=dev)
    if masks is not None:
        tensor_arg(masks, "texture_points: masks", torch.uint8, (m, H, W), device=dev)
    if fallback is not None:
        tensor_arg(fallback, "texture_points: fallback", torch.float32, (n, c), device=dev)
    nv = nf = 0
    if grid is not None:
        if not isinstance(grid, MeshGrid):
            raise L.GpnerfError("texture_points: grid must be a MeshGrid (build_mesh_grid)")
        vertices, faces = grid.vertices, grid.faces
    if vertices is not None or faces is not None:
        nv, nf = mesh_args(vertices, faces, "texture_points", min_faces=1)
        if vertices.device != dev:
            raise L.GpnerfError("texture_points: points and mesh are on different devices")
    nbytes = int(lib.gpnerf_texture_workspace_bytes(n, m))
    if nbytes <= 0 and n > 0:
        raise L.GpnerfError(f"texture_points: refused ({n} points, {m} views)")
    ws = _workspace(dev, max(nbytes, 256))
    res = {"stats": torch.empty((m, L.TEXTURE_FATES), device=dev, dtype=torch.int64), "totals": torch.empty((2,), device=dev, dtype=torch.int64)}
    if "color" in want:
        res["color"] = torch.empty((n, c), device=dev, dtype=torch.float32)
    if "weight" in want:
        res["weight"] = torch.empty((n,), device=dev, dtype=torch.float32)
    if "views" in want:
        res["views"] = torch.empty((n,), device=dev, dtype=torch.uint8)
    bg = np.broadcast_to(np.asarray(background, dtype=np.float32), (c,))
    L.check(lib.gpnerf_texture_points(ptr(points), n, ptr(normals), cams.ctypes.data_as(L.DP), m, images.data_ptr(), H, W, c, ptr(masks),
                                      (vertices.data_ptr() or faces.data_ptr()) if nf else None, nv, faces.data_ptr() if nf else None, nf,
                                      grid.workspace.data_ptr() if grid is not None else None, float(z_near), float(cos_min), int(sharpness),
                                      float(eps), L.TEXTURE_MODES[mode], ptr(fallback), (C.c_float * c)(*[float(b) for b in bg]),
                                      ws.data_ptr(), ws.numel(), ptr(res.get("color")), ptr(res.get("weight")), ptr(res.get("views")),
                                      res["stats"].data_ptr(), res["totals"].data_ptr(), _stream_ptr(dev)), "gpnerf_texture_points")
    return res


def texture_mesh(vertices, faces, Ks, RTs, images, normals=None, grid=None, **kw):
    """texture_points on a device mesh's own vertices, hidden by the mesh itself: the grid is built when none is given (build_mesh_grid,
    whose check is the call's one host read; pass a grid to read nothing), and without normals the area-weighted vertex normals of the
    faces are used (face_vertex_normals).  The keywords are texture_points'."""
    mesh_args(vertices, faces, "texture_mesh", min_faces=1)
    if grid is None:
        grid = build_mesh_grid(vertices, faces)
    elif not isinstance(grid, MeshGrid):
        raise L.GpnerfError("texture_mesh: grid must be a MeshGrid (build_mesh_grid)")
    if normals is None:
        normals = face_vertex_normals(vertices, faces)
    return texture_points(vertices, Ks, RTs, images, normals=normals, grid=grid, **kw)


def read_texture_stats(stats, totals):
    """texture_points' counts on the host (arrays or tensors; the one read, at the end) -> {"per_view": {name: [...]} for _lib.TEXTURE_STATS,
    "used_fraction": [...] per view, "seen", "unseen", "seen_fraction"}; a fraction of nothing is 0."""
    s, seen = host_int64(stats).reshape(-1, L.TEXTURE_FATES), row_dict(totals, ("seen", "unseen"), "read_texture_stats")
    n = seen["seen"] + seen["unseen"]
    res = {"per_view": {name: [int(v) for v in s[:, k]] for k, name in enumerate(L.TEXTURE_STATS)}}
    res["used_fraction"] = [float(u) / n if n else 0.0 for u in s[:, L.TEXTURE_USED]]
    res.update(seen)
    res["seen_fraction"] = float(seen["seen"]) / n if n else 0.0
    return res


def atlas_layout(n_faces, res):
    """gpnerf_atlas_layout (host arithmetic only) -> {name: int} for _lib.ATLAS_LAYOUT: the cells across and down, the image's width and
    height, the texels per face and in all.  Raises for what the atlas calls refuse (res outside 2..64, an image side above 16384,
    2^31 texels or more)."""
    row = (C.c_int64 * len(L.ATLAS_LAYOUT))()
    lib = L.lib()
    try:
        code = lib.gpnerf_atlas_layout(int(n_faces), int(res), row)
    except (C.ArgumentError, OverflowError, TypeError, ValueError):
        code = -1
    if code != 0:
        raise L.GpnerfError(f"atlas_layout: refused ({n_faces} faces, res {res}; res is {L.ATLAS_MIN_RES} to {L.ATLAS_MAX_RES}, the image at most "
                            "16384 x 16384, fewer than 2^31 texels)")
    return dict(zip(L.ATLAS_LAYOUT, (int(v) for v in row)))


def _vertex_rows(t, nv, dev, what, channels=None):
    return tensor_arg(t, what, torch.float32, (nv, channels), device=dev)


def atlas_texels(vertices, faces, res, normals=None, attrs=None, first_face=0, count=None, want=("points", "normals")):
    """gpnerf_atlas_texels: the surface points of the atlas's texels for the faces first_face .. first_face + count - 1 (default: to the
    last) of a device mesh, in global texel order.  Returns a dict of device float32 tensors: "points" [T,3] and "normals" [T,3] as
    `want` names them -- the corners' `normals` (device float32 [nv,3]) combined with the texel's weights, or without them the face's
    cross product, not normalised --, and "attrs" [T,C] when per-vertex `attrs` (device float32 [nv,C], C <= 4) are given.  A face with
    an index out of range gives NaN rows.  Nothing is read back."""
    lib = L.lib()
    vertices, faces = _raster_mesh(vertices, faces, "atlas_texels")
    unknown = set(want) - {"points", "normals"}
    if unknown:
        raise L.GpnerfError(f"atlas_texels: want names {sorted(unknown)}; points and normals are what there is (attrs come with `attrs`)")
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    lay = atlas_layout(nf, res)
    first_face = int(first_face)
    count = nf - first_face if count is None else int(count)
    if first_face < 0 or count < 0 or first_face + count > nf:
        raise L.GpnerfError(f"atlas_texels: faces {first_face} .. {first_face + count - 1} of {nf}")
    if normals is not None:
        _vertex_rows(normals, nv, dev, "atlas_texels: normals", 3)
    c = 1
    if attrs is not None:
        _vertex_rows(attrs, nv, dev, "atlas_texels: attrs")
        c = int(attrs.shape[1])
        if not 1 <= c <= L.TEXTURE_MAX_CHANNELS:
            raise L.GpnerfError(f"atlas_texels: 1 to {L.TEXTURE_MAX_CHANNELS} attribute channels, got {c}")
    n = count * lay["texels_per_face"]
    res_ = {}
    if "points" in want:
        res_["points"] = torch.empty((n, 3), device=dev, dtype=torch.float32)
    if "normals" in want:
        res_["normals"] = torch.empty((n, 3), device=dev, dtype=torch.float32)
    if attrs is not None:
        res_["attrs"] = torch.empty((n, c), device=dev, dtype=torch.float32)
    L.check(lib.gpnerf_atlas_texels(ptr(vertices), nv, ptr(faces), nf, ptr(normals), ptr(attrs), c, int(res), first_face, count,
                                    ptr(res_.get("points")), ptr(res_.get("normals")), ptr(res_.get("attrs")), _stream_ptr(dev)),
            "gpnerf_atlas_texels")
    return res_


class TextureAtlas:
    """texture_atlas' result, device tensors throughout: `image` float32 [Ht,Wt,C] and `coverage` uint8 [Ht,Wt] (_lib.ATLAS_UNOWNED, _SEEN,
    _FALLBACK, _GUTTER), the lists in global texel order `colors` [T,C], `weight` [T] and `views` uint8 [T] (texture_points' outputs
    for the texels), `stats` int64 [m,6] and `totals` int64 [2] counted over TEXELS (read_texture_stats reads them as they are), `res`,
    `n_faces` and `layout` (atlas_layout's dict)."""

    def __init__(self, image, coverage, colors, weight, views, stats, totals, res, n_faces, layout):
        self.image, self.coverage, self.colors, self.weight, self.views = image, coverage, colors, weight, views
        self.stats, self.totals, self.res, self.n_faces, self.layout = stats, totals, int(res), int(n_faces), layout

    def face_uvs(self):
        """host float64 [n_faces,3,2]: the (u, v) of every face's corner texels a, b, c -- texel centres of the image, OBJ's v up"""
        return atlas_face_uvs(self.n_faces, self.res)

    def shade(self, face_id, vertices, faces, Ks, RTs, filter="simplex", background=0.0, z_near=1e-6):
        """gpnerf_atlas_shade: the mesh drawn from this atlas over rasterize_mesh's `face_id` (device int32 [n,H,W], same mesh, cameras
        and z_near) -> device float32 [n,H,W,C]; a pixel no face of its own covers takes `background` (a number or C numbers).
        filter: "simplex" (barycentric on the face's texel lattice) or "nearest".  Only the face's own texels are read."""
        lib = L.lib()
        if filter not in L.ATLAS_FILTERS:
            raise L.GpnerfError(f"TextureAtlas.shade: filter is 'simplex' or 'nearest', got {filter!r}")
        vertices, faces = _raster_mesh(vertices, faces, "TextureAtlas.shade")
        nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
        if nf != self.n_faces or self.image.device != dev:
            raise L.GpnerfError(f"TextureAtlas.shade: the atlas was baked for {self.n_faces} faces on {self.image.device}, got {nf} on {dev}")
        cams = _raster_cams(Ks, RTs, "TextureAtlas.shade")
        n = cams.shape[0]
        tensor_arg(face_id, "TextureAtlas.shade: face_id", torch.int32, (n, None, None), device=dev)
        H, W = int(face_id.shape[1]), int(face_id.shape[2])
        c = int(self.image.shape[2])
        bg = np.broadcast_to(np.asarray(background, dtype=np.float32), (c,))
        out = torch.empty((n, H, W, c), device=dev, dtype=torch.float32)
        L.check(lib.gpnerf_atlas_shade(face_id.data_ptr(), ptr(vertices), nv, ptr(faces), nf, cams.ctypes.data_as(L.DP), n, H, W, float(z_near),
                                       ptr(self.image), self.res, c, L.ATLAS_FILTERS[filter], (C.c_float * c)(*[float(b) for b in bg]),
                                       out.data_ptr(), _stream_ptr(dev)), "gpnerf_atlas_shade")
        return out


def atlas_face_uvs(n_faces, res):
    """host float64 [n_faces,3,2]: (u, v) of the corner texels a = (0, 0), b = (res - 1, 0), c = (0, res - 1) of every face under the
    packing of include/gpnerf_hip.h: u = (X + 0.5) / Wt, v = 1 - (Y + 0.5) / Ht"""
    lay = atlas_layout(n_faces, res)
    R = int(res)
    f = np.arange(int(n_faces), dtype=np.int64)
    q, odd = f // 2, (f % 2).astype(bool)
    i, j = np.array([0, R - 1, 0], np.int64), np.array([0, 0, R - 1], np.int64)
    x = np.where(odd[:, None], R + 1 - i[None], i[None])
    y = np.where(odd[:, None], R - 1 - j[None], j[None])
    cx = max(lay["cells_x"], 1)
    X, Y = (q % cx)[:, None] * (R + 2) + x, (q // cx)[:, None] * R + y
    return np.stack([(X + 0.5) / max(lay["width"], 1), 1.0 - (Y + 0.5) / max(lay["height"], 1)], axis=-1)


def atlas_pack(colors, views, n_faces, res, background=0.0):
    """gpnerf_atlas_pack: the colour list (device float32 [T,C], global texel order) into the image -> (image float32 [Ht,Wt,C],
    coverage uint8 [Ht,Wt]).  views: device uint8 [T] (a texel whose bits are 0 is on its fallback) or None.  A gather: every image
    texel reads its owner's row; a gutter texel takes the mean of its owned neighbours, an unowned one `background`."""
    lib = L.lib()
    lay = atlas_layout(n_faces, res)
    t = lay["n_texels"]
    tensor_arg(colors, "atlas_pack: colors", torch.float32, (t, None))
    dev, c = colors.device, int(colors.shape[1])
    if not 1 <= c <= L.TEXTURE_MAX_CHANNELS:
        raise L.GpnerfError(f"atlas_pack: 1 to {L.TEXTURE_MAX_CHANNELS} channels, got {c}")
    if views is not None:
        tensor_arg(views, "atlas_pack: views", torch.uint8, (t,), device=dev)
    bg = np.broadcast_to(np.asarray(background, dtype=np.float32), (c,))
    image = torch.empty((lay["height"], lay["width"], c), device=dev, dtype=torch.float32)
    coverage = torch.empty((lay["height"], lay["width"]), device=dev, dtype=torch.uint8)
    L.check(lib.gpnerf_atlas_pack(ptr(colors), ptr(views), int(n_faces), int(res), c, (C.c_float * c)(*[float(b) for b in bg]), ptr(image),
                                  ptr(coverage), _stream_ptr(dev)), "gpnerf_atlas_pack")
    return image, coverage


def texture_atlas(vertices, faces, Ks, RTs, images, res=8, normals=None, masks=None, grid=None, fallback=None, chunk_texels=1 << 20,
                  background=0.0, **kw):
    """A per-face texture atlas of a device mesh baked from calibrated views -> TextureAtlas.  The faces are walked in chunks of at
    most chunk_texels texels (at least one face): atlas_texels gives the chunk's surface points and normals (the corners' `normals`,
    device float32 [nv,3], combined; without them the faces' own), texture_points colours them -- UNCHANGED: Ks, RTs, images, masks and
    the keywords mode, sharpness, cos_min, eps, z_near are its, the mesh hides its own texels through `grid` (built when none is
    given, as texture_mesh does: build_mesh_grid's check is then the call's one host read) -- into slices of one colour, weight and
    view-bits list, the counts are added on the device, and atlas_pack makes the image.  fallback: per-VERTEX colours, device float32
    [nv,C], spread over the texels by atlas_texels: what a texel no view sees keeps (without it: background).  A chunked bake equals
    an unchunked one bit for bit; the chunk bounds texture_points' workspace (49 bytes per texel and view)."""
    nv, nf = mesh_args(vertices, faces, "texture_atlas", min_faces=1)
    dev = vertices.device
    for name in ("vertices", "faces", "want", "points"):
        if name in kw:
            raise L.GpnerfError(f"texture_atlas: {name} is not a keyword of the bake")
    lay = atlas_layout(nf, res)
    tpf, t = lay["texels_per_face"], lay["n_texels"]
    if int(chunk_texels) < 1:
        raise L.GpnerfError(f"texture_atlas: chunk_texels must be at least 1, got {chunk_texels}")
    if grid is None:
        grid = build_mesh_grid(vertices, faces)
    elif not isinstance(grid, MeshGrid):
        raise L.GpnerfError("texture_atlas: grid must be a MeshGrid (build_mesh_grid)")
    tensor_arg(images, "texture_atlas: images", torch.float32, (None, None, None, None), device=dev)
    m, c = int(images.shape[0]), int(images.shape[3])
    if fallback is not None:
        _vertex_rows(fallback, nv, dev, "texture_atlas: fallback", c)
    colors = torch.empty((t, c), device=dev, dtype=torch.float32)
    weight = torch.empty((t,), device=dev, dtype=torch.float32)
    views = torch.empty((t,), device=dev, dtype=torch.uint8)
    stats = torch.zeros((m, L.TEXTURE_FATES), device=dev, dtype=torch.int64)
    totals = torch.zeros((2,), device=dev, dtype=torch.int64)
    per = max(1, int(chunk_texels) // tpf)
    for first in range(0, nf, per):
        count = min(per, nf - first)
        tex = atlas_texels(vertices, faces, res, normals=normals, attrs=fallback, first_face=first, count=count)
        got = texture_points(tex["points"], Ks, RTs, images, normals=tex["normals"], masks=masks, grid=grid, fallback=tex.get("attrs"),
                             background=background, **kw)
        rows = slice(first * tpf, (first + count) * tpf)
        colors[rows], weight[rows], views[rows] = got["color"], got["weight"], got["views"]
        stats += got["stats"]
        totals += got["totals"]
    image, coverage = atlas_pack(colors, views, nf, res, background=background)
    return TextureAtlas(image, coverage, colors, weight, views, stats, totals, res, nf, lay)
