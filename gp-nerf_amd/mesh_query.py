"""Points and rays against a mesh: distances, samples, registration, metrics and ray casts (csrc/gpnerf_meshdist.hip, gpnerf_align.hip,
gpnerf_raycast.hip).

In: a device mesh of at least one face -- contiguous float32 vertices [n,3], int32 faces [m,3]; mesh_to_device uploads a mesh.Mesh --
or its MeshGrid (build_mesh_grid), and device float32 points [n,3] or rays [...,8].  Out, all on the device: per point the distance,
nearest face and point (point_mesh_distance); surface samples (sample_surface); reductions in float64 slots (distance_stats,
mesh_metrics); rigid transforms in float64 slots (rigid_fit, align_mesh and its steps; transform_points applies one); per ray the hit
(raycast_mesh, mesh_visibility; pixel_rays makes a camera's rays).  The read_* functions turn a slot into a dict on the host.  frame
re-exports every public name."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._args import _points, _raster_cams, _stream_ptr, mesh_args, mesh_to_device, ptr, tensor_arg


def mesh_grid_caps(n_faces):
    """The default capacities of build_mesh_grid, from n_faces alone: cell_cap = n_faces clamped to [64, 2^22] -- about one cell per
    face, so a marching-cubes triangle (no longer than a voxel's diagonal) overlaps 1 - 8 cells and a cell's run stays a few entries
    long; entry_cap = 8 n_faces + 4 cell_cap -- eight cells per face, plus room for the few large faces of a hand-made mesh.  A
    mesh whose faces are large against its cells (one face across the whole box lands in every cell) can need more: the build reports
    the count and build_mesh_grid retries with it."""
    cell_cap = int(min(max(n_faces, 64), 1 << 22))
    return cell_cap, 8 * int(n_faces) + 4 * cell_cap


class MeshGrid:
    """gpnerf_mesh_grid_build's workspace with the mesh it was built for.  `header()` reads the header words (one device-to-host
    copy): status, skipped, valid, cells [3], n_cells, cell_cap, entry_cap, needed, lo / size / inv [3] float32."""

    def __init__(self, vertices, faces, workspace, cell_cap, entry_cap):
        self.vertices, self.faces, self.workspace, self.cell_cap, self.entry_cap = vertices, faces, workspace, cell_cap, entry_cap

    def header(self):
        w = self.workspace[:4 * L.GRID_HDR_INTS].cpu().numpy().view(np.int32)
        H = L.GRID_HDR
        res = {k: int(w[H[k]]) for k in ("status", "skipped", "valid", "n_cells", "cell_cap", "entry_cap")}
        res["cells"] = [int(v) for v in w[H["cells"]:H["cells"] + 3]]
        res["needed"] = int(w[H["needed"]:H["needed"] + 2].view(np.int64)[0])
        for k in ("lo", "size", "inv"):
            res[k] = w[H[k]:H[k] + 3].view(np.float32).copy()
        return res


def build_mesh_grid(vertices, faces, cell_cap=None, entry_cap=None, check=True):
    """gpnerf_mesh_grid_build on a device mesh (float32 [n,3], int32 [m,3]) -> MeshGrid.  Capacities default by mesh_grid_caps.
    check (default): the header's status is read -- the call's one host read -- and on overflow the build runs once more with the
    count the header reports (already in that read); a second overflow raises.  check=False enqueues only: an overflowed grid then
    makes every distance NaN, which read_mesh_metrics reports."""
    lib = L.lib()
    nv, nf = mesh_args(vertices, faces, "build_mesh_grid", min_faces=1)
    d_cell, d_entry = mesh_grid_caps(nf)
    cell_cap, entry_cap = int(cell_cap or d_cell), int(entry_cap or d_entry)
    dev = vertices.device
    for attempt in (0, 1):
        nbytes = int(lib.gpnerf_mesh_grid_workspace_bytes(nf, cell_cap, entry_cap))
        if nbytes <= 0:
            raise L.GpnerfError(f"build_mesh_grid: refused ({nf} faces, cell_cap {cell_cap}, entry_cap {entry_cap})")
        ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        L.check(lib.gpnerf_mesh_grid_build(vertices.data_ptr() or ws.data_ptr(), nv, faces.data_ptr(), nf, cell_cap, entry_cap, ws.data_ptr(),
                                           ws.numel(), _stream_ptr(dev)), "gpnerf_mesh_grid_build")
        grid = MeshGrid(vertices, faces, ws, cell_cap, entry_cap)
        if not check:
            return grid
        h = grid.header()
        if h["status"] == L.GRID_OK:
            return grid
        if attempt or h["status"] != L.GRID_OVERFLOW:
            raise L.GpnerfError(f"build_mesh_grid: status {h['status']}, {h['needed']} entries needed, capacity {entry_cap}")
        entry_cap = h["needed"]


def point_mesh_distance(points, vertices=None, faces=None, grid=None, max_dist=float("inf"), query_normals=None, want_closest=False):
    """gpnerf_mesh_distance: for device float32 points [n,3] the exact distance to the mesh, the nearest face (lowest index among
    equal distances), optionally the nearest point and |n_q . n_f| -> {"dist" [n], "face" int32 [n], "closest" [n,3], "cosine" [n]}.
    grid: a MeshGrid (its mesh is used); without one, `vertices` and `faces` go through the brute-force form.  Nothing is read back."""
    lib = L.lib()
    if grid is not None:
        vertices, faces = grid.vertices, grid.faces
    nv, nf = mesh_args(vertices, faces, "point_mesh_distance", min_faces=1)
    points = _points(points, "point_mesh_distance: points", device=vertices.device)
    if query_normals is not None:
        query_normals = _points(query_normals, "point_mesh_distance: query_normals", like=points)
    n, dev = int(points.shape[0]), points.device
    res = {"dist": torch.empty((n,), device=dev, dtype=torch.float32), "face": torch.empty((n,), device=dev, dtype=torch.int32)}
    if want_closest:
        res["closest"] = torch.empty((n, 3), device=dev, dtype=torch.float32)
    if query_normals is not None:
        res["cosine"] = torch.empty((n,), device=dev, dtype=torch.float32)
    L.check(lib.gpnerf_mesh_distance(ptr(points), n, vertices.data_ptr() or faces.data_ptr(), nv, faces.data_ptr(), nf,
                                     grid.workspace.data_ptr() if grid is not None else None, float(max_dist),
                                     (query_normals.data_ptr() or faces.data_ptr()) if query_normals is not None else None, ptr(res["dist"]),
                                     ptr(res["face"]), ptr(res.get("closest")),
                                     (res["cosine"].data_ptr() or faces.data_ptr()) if query_normals is not None else None,
                                     _stream_ptr(dev)), "gpnerf_mesh_distance")
    return res


def sample_surface(vertices, faces, n_samples, seed=0, want_face=True, want_normal=True):
    """gpnerf_mesh_sample_surface: n_samples deterministic, stratified, area-weighted points on a device mesh ->
    {"points" [n,3], "face" int32 [n], "normal" [n,3], "workspace"} (the workspace's first int32 is the status: 1 when the mesh has
    no area, every point NaN then).  Nothing is read back."""
    lib = L.lib()
    nv, nf = mesh_args(vertices, faces, "sample_surface", min_faces=1)
    n, dev = int(n_samples), vertices.device
    nbytes = int(lib.gpnerf_mesh_sample_workspace_bytes(nf))
    if nbytes <= 0 or n < 0:
        raise L.GpnerfError(f"sample_surface: refused ({nf} faces, {n} samples)")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    res = {"points": torch.empty((n, 3), device=dev, dtype=torch.float32), "workspace": ws}
    if want_face:
        res["face"] = torch.empty((n,), device=dev, dtype=torch.int32)
    if want_normal:
        res["normal"] = torch.empty((n, 3), device=dev, dtype=torch.float32)
    L.check(lib.gpnerf_mesh_sample_surface(vertices.data_ptr() or ws.data_ptr(), nv, faces.data_ptr(), nf, n, int(seed) & 0xffffffff, ws.data_ptr(),
                                           ws.numel(), ptr(res["points"]), ptr(res.get("face")), ptr(res.get("normal")), _stream_ptr(dev)),
            "gpnerf_mesh_sample_surface")
    return res


def distance_stats(values, thresholds=(), out=None):
    """gpnerf_distance_stats: one slot (float64 [_lib.DIST_DOUBLES], device) from a device float32 list; out: a slot to write into"""
    lib = L.lib()
    tensor_arg(values, "distance_stats: values", torch.float32)
    th = [float(t) for t in thresholds]
    if len(th) > L.DIST_MAX_THRESHOLDS:
        raise L.GpnerfError(f"distance_stats: at most {L.DIST_MAX_THRESHOLDS} thresholds")
    if out is None:
        out = torch.empty((L.DIST_DOUBLES,), device=values.device, dtype=torch.float64)
    n = values.numel()
    L.check(lib.gpnerf_distance_stats(ptr(values), n, (C.c_float * len(th))(*th) if th else None, len(th), out.data_ptr(),
                                      _stream_ptr(values.device)), "gpnerf_distance_stats")
    return out


def align_workspace(device):
    """a workspace for rigid_fit / align_mesh's calls (uint8, gpnerf_align_workspace_bytes()); _lib.ALIGN_WS names its doubles"""
    return torch.empty((int(L.lib().gpnerf_align_workspace_bytes()),), device=device, dtype=torch.uint8)


def _slot(out, device, what):
    if out is None:
        return torch.empty((L.XFORM_DOUBLES,), device=device, dtype=torch.float64)
    tensor_arg(out, f"{what}: the slot", torch.float64, device=device)
    if out.numel() != L.XFORM_DOUBLES:
        raise L.GpnerfError(f"{what}: the slot holds {L.XFORM_DOUBLES} doubles, got {tuple(out.shape)}")
    return out


def rigid_fit(src, dst, weights=None, scale=False, out=None, workspace=None):
    """gpnerf_rigid_fit: the weighted least-squares x -> s R x + t (s = 1 unless scale) that takes the device float32 points src
    [n,3] onto dst [n,3]; weights: device float32 [n] or None.  Returns the transform slot (float64 [_lib.XFORM_DOUBLES] on the
    device; out: a slot to write into); read_transform turns it into a dict.  workspace: an align_workspace to use (its sums stay
    readable behind the call).  Nothing is read back."""
    lib = L.lib()
    src = _points(src, "rigid_fit: src")
    n, dev = int(src.shape[0]), src.device
    dst = _points(dst, "rigid_fit: dst", like=src, device=dev)
    if weights is not None:
        tensor_arg(weights, "rigid_fit: weights", torch.float32, (n,), device=dev)
    slot = _slot(out, dev, "rigid_fit")
    ws = align_workspace(dev) if workspace is None else workspace
    L.check(lib.gpnerf_rigid_fit(src.data_ptr() or ws.data_ptr(), dst.data_ptr() or ws.data_ptr(),
                                 (weights.data_ptr() or ws.data_ptr()) if weights is not None else None, n, int(bool(scale)), slot.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "gpnerf_rigid_fit")
    return slot


def transform_points(points, slot, vectors=False, out=None):
    """gpnerf_transform_points: float32(M p) for device float32 points [n,3] and a transform slot; vectors: the rotation alone
    (normals).  out: where to write (may be `points` itself).  Nothing is read back."""
    lib = L.lib()
    points = _points(points, "transform_points: points")
    slot = _slot(slot, points.device, "transform_points")
    out = torch.empty_like(points) if out is None else _points(out, "transform_points: out", like=points, device=points.device)
    n = int(points.shape[0])
    L.check(lib.gpnerf_transform_points(points.data_ptr() or slot.data_ptr(), n, slot.data_ptr(), int(bool(vectors)),
                                        out.data_ptr() or slot.data_ptr(), _stream_ptr(points.device)), "gpnerf_transform_points")
    return out


def read_transform(slot):
    """A transform slot (tensor or array; the tensor's copy is the one host read, and the caller's) -> dict: matrix (4 x 4 float64),
    scale, rotation_deg (the angle of R), translation [3], rms, used, skipped, trimmed, status ("ok", "few", "singular"), pivot [3].
    Raises when nothing was used and every pair was skipped: align_mesh's target grid overflowed its entry capacity, or the
    sampled mesh has no valid face with area (read_mesh_metrics' advice)."""
    s = np.asarray(slot.detach().cpu() if isinstance(slot, torch.Tensor) else slot, dtype=np.float64).reshape(L.XFORM_DOUBLES)
    used, skipped, trimmed = (int(s[k]) for k in (L.XFORM_USED, L.XFORM_SKIPPED, L.XFORM_TRIMMED))
    if used == 0 and trimmed == 0 and skipped > 0:
        raise L.GpnerfError("read_transform: every pair was skipped: either the grid of the mesh registered onto overflowed its "
                            "entry capacity (build_mesh_grid(vertices, faces).entry_cap is a capacity that fits: pass it as entry_cap), "
                            "or the sampled mesh has no valid face with a positive area")
    M = np.vstack([s[L.XFORM_M:L.XFORM_M + 12].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
    scale = float(s[L.XFORM_SCALE])
    cos = (np.trace(M[:3, :3]) / scale - 1.0) / 2.0
    return {"matrix": M, "scale": scale, "rotation_deg": float(np.degrees(np.arccos(min(1.0, max(-1.0, cos))))),
            "translation": M[:3, 3].copy(), "rms": float(s[L.XFORM_RMS]), "used": used, "skipped": skipped, "trimmed": trimmed,
            "status": L.ALIGN_STATUS_NAMES[int(s[L.XFORM_STATUS])], "pivot": s[L.XFORM_PIVOT:L.XFORM_PIVOT + 3].copy()}


def align_init(points, init=None, out=None, workspace=None):
    """gpnerf_align_init: a slot with M = init (a host 3 x 4 or 4 x 4 matrix; None: the identity) and PIVOT = the centroid of the
    finite device float32 points [n,3]"""
    lib = L.lib()
    points = _points(points, "align_init: points")
    dev = points.device
    slot = _slot(out, dev, "align_init")
    ws = align_workspace(dev) if workspace is None else workspace
    m = None
    if init is not None:
        a = np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
        if a.shape not in ((3, 4), (4, 4)):
            raise L.GpnerfError(f"align_init: init is a 3 x 4 or 4 x 4 matrix, got {a.shape}")
        m = (C.c_double * 12)(*a[:3].reshape(-1))
    L.check(lib.gpnerf_align_init(points.data_ptr() or ws.data_ptr(), int(points.shape[0]), m, slot.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _stream_ptr(dev)), "gpnerf_align_init")
    return slot


def align_step(cur, nearest, vertices, faces, slot, max_dist=float("inf"), history_row=None, workspace=None):
    """gpnerf_align_step: one trimmed point-to-plane step composed onto the slot's matrix.  cur: the source points as transformed by
    the slot; nearest: point_mesh_distance(cur, ..., want_closest=True)'s result against the device mesh (vertices, faces);
    history_row: a device float64 [4] for (rms, used, trimmed, status)."""
    lib = L.lib()
    nv, nf = mesh_args(vertices, faces, "align_step", min_faces=1)
    cur = _points(cur, "align_step: cur")
    dev = cur.device
    closest = _points(nearest["closest"], "align_step: closest", like=cur)
    face, dist = nearest["face"], nearest["dist"]
    n = int(cur.shape[0])
    if face.dtype != torch.int32 or dist.dtype != torch.float32 or face.shape != (n,) or dist.shape != (n,) or not face.is_contiguous() \
            or not dist.is_contiguous() or any(t.device != dev for t in (closest, face, dist, vertices)):
        raise L.GpnerfError("align_step: face int32 [n] and dist float32 [n] as point_mesh_distance wrote them, on the points' device")
    slot = _slot(slot, dev, "align_step")
    if history_row is not None and (history_row.dtype != torch.float64 or history_row.numel() != 4 or not history_row.is_contiguous()
                                    or history_row.device != dev):
        raise L.GpnerfError("align_step: history_row is a contiguous float64 [4] tensor on the points' device")
    ws = align_workspace(dev) if workspace is None else workspace
    p = lambda t: t.data_ptr() or ws.data_ptr()
    L.check(lib.gpnerf_align_step(p(cur), p(closest), p(face), p(dist), n, p(vertices), nv, faces.data_ptr(), nf, float(max_dist),
                                  slot.data_ptr(), history_row.data_ptr() if history_row is not None else None, ws.data_ptr(), ws.numel(),
                                  _stream_ptr(dev)), "gpnerf_align_step")
    return slot


def align_mesh(src, dst, iterations=10, n_samples=20000, max_dist=float("inf"), seed=0, init=None, grid=None, cell_cap=None,
               entry_cap=None, points=None, device=None):
    """Register the mesh src onto the mesh dst by trimmed point-to-plane ICP, enqueued on the device without a host read:
    n_samples stratified surface samples of src (sample_surface, `seed`), a grid of dst (build_mesh_grid(check=False), unless a
    MeshGrid `grid` of it is given -- dst may then be None), align_init (init: a host 3 x 4 or 4 x 4 starting matrix), then
    `iterations` times, a fixed count: transform_points of the ORIGINAL samples by the cumulative matrix (float32 roundings never
    pile up), point_mesh_distance(want_closest=True) at max_dist inf, align_step (pairs farther than max_dist trimmed).
    points: device float32 [n,3] source points to use instead of sampling (src may then be None).
    src, dst: mesh.Mesh, or (vertices, faces) arrays / tensors.  Returns {"transform": the slot of the transform src -> dst,
    "history": float64 [iterations, 4] on the device, a row (rms before the step, used, trimmed, status) per iteration}.
    A grid that overflowed makes every distance NaN: every pair is skipped, the status is "few", and read_transform raises."""
    if device is None:
        first = points if points is not None else (grid.vertices if grid is not None else (src[0] if isinstance(src, (tuple, list)) else None))
        device = first.device if isinstance(first, torch.Tensor) and first.is_cuda else torch.device("cuda:0")
    device = torch.device(device)
    if device.type != "cuda":
        raise L.GpnerfError(f"align_mesh computes on the GPU (got {device}); the HIP path has no CPU fallback")
    iterations = int(iterations)
    if iterations < 0:
        raise L.GpnerfError(f"align_mesh: iterations >= 0, got {iterations}")
    if points is None:
        sv, sf = mesh_to_device(src, device)
        points = sample_surface(sv, sf, n_samples, seed=seed, want_face=False, want_normal=False)["points"]
    points = _points(points, "align_mesh: points")
    if grid is None:
        dv, df = mesh_to_device(dst, device)
        grid = build_mesh_grid(dv, df, cell_cap, entry_cap, check=False)
    ws = align_workspace(device)
    slot = align_init(points, init, workspace=ws)
    history = torch.empty((iterations, 4), device=device, dtype=torch.float64)
    cur = torch.empty_like(points)
    for it in range(iterations):
        transform_points(points, slot, out=cur)
        near = point_mesh_distance(cur, grid=grid, want_closest=True)
        align_step(cur, near, grid.vertices, grid.faces, slot, max_dist=max_dist, history_row=history[it], workspace=ws)
    return {"transform": slot, "history": history}


MESH_METRIC_ROWS = ("pred_to_gt", "gt_to_pred", "cos_pred_to_gt", "cos_gt_to_pred")
ALIGN_SAMPLES = 20000                    # align_mesh's default number of source samples


def mesh_metrics(pred, gt, n_samples=100000, thresholds=(0.005, 0.01, 0.02), seed=0, max_dist=float("inf"), device=None, cell_cap=None,
                 entry_cap=None, align=None, align_iterations=10, align_max_dist=float("inf"), want_transform=False):
    """The geometry metrics of a predicted mesh against a ground-truth one, enqueued on the device without a host read:
    n_samples stratified surface samples of each (sample_surface; seeds `seed` and `seed + 1`), the exact distance of each sample
    to the OTHER mesh with the cosine between the sample's face normal and the nearest face's (point_mesh_distance through a grid
    built with check=False), and the four reductions (distance_stats).  pred, gt: mesh.Mesh, or (vertices, faces) arrays / tensors,
    in the same frame and unit; device: where to compute (default: the tensors' device, else cuda:0).
    align: None (the default: the meshes are compared where they are, with exactly the launches of a call without the keyword), or
    "rigid": the predicted mesh is first registered onto gt by align_mesh (align_iterations steps on min(n_samples, ALIGN_SAMPLES)
    samples, pairs beyond align_max_dist trimmed) and its vertices go through transform_points before the sampling: still no host
    read.  want_transform: return (slots, transform slot); the slot is None without align.
    Returns float64 [4, _lib.DIST_DOUBLES] on the device, rows MESH_METRIC_ROWS; read_mesh_metrics turns it into a dict."""
    if align not in (None, "rigid"):
        raise L.GpnerfError(f"mesh_metrics: align is None or 'rigid', got {align!r}")
    if device is None:
        v = pred[0] if isinstance(pred, (tuple, list)) else None
        device = v.device if isinstance(v, torch.Tensor) and v.is_cuda else torch.device("cuda:0")
    device = torch.device(device)
    if device.type != "cuda":
        raise L.GpnerfError(f"mesh_metrics computes on the GPU (got {device}); the HIP path has no CPU fallback")
    th = tuple(float(t) for t in thresholds)
    pv, pf = mesh_to_device(pred, device)
    gv, gf = mesh_to_device(gt, device)
    slots = torch.empty((4, L.DIST_DOUBLES), device=device, dtype=torch.float64)
    transform = g_gt = None
    if align is not None:
        g_gt = build_mesh_grid(gv, gf, cell_cap, entry_cap, check=False)
        transform = align_mesh((pv, pf), None, iterations=align_iterations, n_samples=min(int(n_samples), ALIGN_SAMPLES),
                               max_dist=align_max_dist, seed=seed, grid=g_gt)["transform"]
        pv = transform_points(pv, transform)
    sp = sample_surface(pv, pf, n_samples, seed=seed, want_face=False)
    sg = sample_surface(gv, gf, n_samples, seed=seed + 1, want_face=False)
    if g_gt is None:
        g_gt = build_mesh_grid(gv, gf, cell_cap, entry_cap, check=False)
    g_pred = build_mesh_grid(pv, pf, cell_cap, entry_cap, check=False)
    a = point_mesh_distance(sp["points"], grid=g_gt, max_dist=max_dist, query_normals=sp["normal"])
    b = point_mesh_distance(sg["points"], grid=g_pred, max_dist=max_dist, query_normals=sg["normal"])
    distance_stats(a["dist"], th, out=slots[0])
    distance_stats(b["dist"], th, out=slots[1])
    distance_stats(a["cosine"], (), out=slots[2])
    distance_stats(b["cosine"], (), out=slots[3])
    return (slots, transform) if want_transform else slots


def read_mesh_metrics(slots, thresholds=(0.005, 0.01, 0.02)):
    """mesh_metrics' slots (one [4, DIST_DOUBLES] tensor or array) -> dict, in the meshes' own unit: accuracy (mean distance pred ->
    gt, the usual P2S), completeness (gt -> pred), chamfer (half their sum), normal_consistency (the mean of the two cosine means),
    per threshold t precision@t, recall@t (the fractions within t) and fscore@t (their harmonic mean, 0 when both are 0),
    accuracy_max, completeness_max, and the counts n_pred / n_gt (finite), beyond_pred / beyond_gt (past max_dist), nan_pred / nan_gt.
    Raises when a direction has nothing but NaN: its grid overflowed (pass entry_cap) or the sampled mesh has no valid face with area."""
    s = np.asarray(slots.detach().cpu() if isinstance(slots, torch.Tensor) else slots, dtype=np.float64).reshape(4, L.DIST_DOUBLES)
    for row, name in ((0, "pred -> gt"), (1, "gt -> pred")):
        if s[row, L.DIST_NAN] > 0 and s[row, L.DIST_FINITE] + s[row, L.DIST_INF] == 0:
            raise L.GpnerfError(f"mesh_metrics: every distance {name} is NaN: either the grid of the mesh measured against overflowed its "
                                "entry capacity (build_mesh_grid(vertices, faces).entry_cap is a capacity that fits: pass it as entry_cap), "
                                "or the sampled mesh has no valid face with a positive area")
    res = {"accuracy": float(s[0, L.DIST_MEAN]), "completeness": float(s[1, L.DIST_MEAN])}
    res["chamfer"] = 0.5 * (res["accuracy"] + res["completeness"])
    res["normal_consistency"] = 0.5 * float(s[2, L.DIST_MEAN] + s[3, L.DIST_MEAN])
    for k, t in enumerate(thresholds):
        p, r = float(s[0, L.DIST_WITHIN + k]), float(s[1, L.DIST_WITHIN + k])
        res[f"precision@{t:g}"], res[f"recall@{t:g}"] = p, r
        res[f"fscore@{t:g}"] = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    res["accuracy_max"], res["completeness_max"] = float(s[0, L.DIST_MAX]), float(s[1, L.DIST_MAX])
    for row, name in ((0, "pred"), (1, "gt")):
        res[f"n_{name}"], res[f"beyond_{name}"], res[f"nan_{name}"] = (int(s[row, k]) for k in (L.DIST_FINITE, L.DIST_INF, L.DIST_NAN))
    return res


def raycast_mesh(rays, vertices=None, faces=None, grid=None, mode="nearest", want_bary=False):
    """gpnerf_mesh_raycast: what each ray of a device float32 [...,8] list of (o, d, tmin, tmax) rows -- make_rays' and render_fused's
    layout, d as given, so t is the renderer's depth -- hits of the mesh -> {"t" [...], "face" int32 [...], "bary" [...,2]}.
    mode "nearest": the smallest t in [tmin, tmax] (+inf: none; NaN: a ray that is not one), its face (the lowest index among equal
    t, -1: none) and, with want_bary, the hit's barycentric weights of the face's second and third vertex.  mode "any": t = 0 where
    some face lies in [tmin, tmax] and +inf where none does -- a shadow ray; which face it names depends on the form.
    grid: a MeshGrid (its mesh is used) selects the walk through the grid; without one, `vertices` and `faces` go through the
    brute-force form; the two agree bit for bit.  Nothing is read back."""
    lib = L.lib()
    if mode not in L.RAYCAST_MODES:
        raise L.GpnerfError(f"raycast_mesh: mode is 'nearest' or 'any', got {mode!r}")
    if grid is not None:
        if not isinstance(grid, MeshGrid):
            raise L.GpnerfError("raycast_mesh: grid must be a MeshGrid (build_mesh_grid)")
        vertices, faces = grid.vertices, grid.faces
    nv, nf = mesh_args(vertices, faces, "raycast_mesh", min_faces=1)
    tensor_arg(rays, "raycast_mesh: rays", torch.float32, (..., 8), device=vertices.device)      # rows of (o, d, tmin, tmax)
    shape, dev = tuple(rays.shape[:-1]), rays.device
    n = int(np.prod(shape, dtype=np.int64))
    res = {"t": torch.empty(shape, device=dev, dtype=torch.float32), "face": torch.empty(shape, device=dev, dtype=torch.int32)}
    if want_bary:
        res["bary"] = torch.empty(shape + (2,), device=dev, dtype=torch.float32)
    L.check(lib.gpnerf_mesh_raycast(ptr(rays), n, vertices.data_ptr() or faces.data_ptr(), nv, faces.data_ptr(), nf,
                                    grid.workspace.data_ptr() if grid is not None else None, L.RAYCAST_MODES[mode], ptr(res["t"]),
                                    ptr(res["face"]), ptr(res.get("bary")), _stream_ptr(dev)), "gpnerf_mesh_raycast")
    return res


def pixel_rays(Ks, RTs, H, W, z_near=1e-6, device=None):
    """gpnerf_pixel_rays: the rays through the pixel centres of the cameras Ks [n,3,3], RTs [n,3,4] (host arrays, used in float64;
    rasterize_mesh's cameras and pixel convention) -> device float32 [n,H,W,8] rows (o, d, z_near, +inf) with d's camera-z component 1:
    raycast_mesh's t along them is the camera depth rasterize_mesh draws.  device: where the rays go (default cuda:0)."""
    lib = L.lib()
    cams = _raster_cams(Ks, RTs, "pixel_rays")
    dev = torch.device(device if device is not None else "cuda:0")
    if dev.type != "cuda":
        raise L.GpnerfError(f"pixel_rays: the rays must live on the GPU (got {dev}); the HIP path has no CPU fallback")
    n, H, W = cams.shape[0], int(H), int(W)
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise L.GpnerfError(f"pixel_rays: refused ({n} views, {H} x {W})")
    rays = torch.empty((n, H, W, 8), device=dev, dtype=torch.float32)
    L.check(lib.gpnerf_pixel_rays(cams.ctypes.data_as(L.DP), n, H, W, float(z_near), rays.data_ptr(), _stream_ptr(dev)), "gpnerf_pixel_rays")
    return rays


def mesh_visibility(points, eyes, vertices=None, faces=None, grid=None, eps=1e-4):
    """Which of the device float32 points [n,3] each of the eyes [m,3] (device float32, or host numbers) sees past the mesh ->
    device uint8 [n,m], 1 where nothing lies between.  One "any" ray per pair: o = p, d = eye - p, tmin = eps, tmax = 1, so the
    segment from just off the point to the eye; eps (a fraction of the segment) keeps a point ON the mesh from being hidden by its
    own faces.  The rows are composed by torch; the cast is raycast_mesh's.  Nothing is read back."""
    points = _points(points, "mesh_visibility: points")
    dev = points.device
    eyes = torch.as_tensor(eyes, dtype=torch.float32).to(dev).reshape(-1, 3)
    n, m = int(points.shape[0]), int(eyes.shape[0])
    rows = torch.empty((n, m, 8), device=dev, dtype=torch.float32)
    rows[..., 0:3] = points[:, None, :]
    rows[..., 3:6] = eyes[None, :, :] - points[:, None, :]
    rows[..., 6] = float(eps)
    rows[..., 7] = 1.0
    t = raycast_mesh(rows, vertices, faces, grid=grid, mode="any")["t"]
    return (t > 0).to(torch.uint8)
