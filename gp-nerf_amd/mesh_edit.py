"""Mesh in, mesh out: the tools that change a device mesh or report on its connectivity.

In: a device mesh -- contiguous float32 vertices [n,3] and int32 faces [m,3] on one device (mesh_to_device uploads a mesh.Mesh).
Out: a new device mesh with device stats (simplify_mesh: quadric vertex clustering; filter_components: the kept connected
components; repair_mesh: weld, de-duplicate, orient outward), new vertices (smooth_mesh: Taubin), or a report that stays on the
device (mesh_adjacency / mesh_topology, mesh_components); the read_* functions name a report's counts on the host, the parse_*
functions read the knobs extract_mesh and the Renderer pass on.  frame re-exports every public name."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L
from ._args import _stream_ptr, host_int64, mesh_args, mesh_to_device, ptr, row_dict, rows3_arg, view


def parse_simplify(value, what="simplify"):
    """extract_mesh(simplify=...) / Renderer(mesh_simplify=...) / GPNERF_MESH_SIMPLIFY -> None (off) or the cell edge in lattice steps, a
    float > 0: off is None, False, 0, "0" or ""; anything else that is not a finite number > 0 is refused."""
    if value is None or value is False:
        return None
    if isinstance(value, str):
        text = value.strip()
        if text in ("", "0"):
            return None
        try:
            value = float(text)
        except ValueError:
            raise L.GpnerfError(f"{what}: expected 0 or a cell edge in lattice steps > 0, got {text!r}") from None
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise L.GpnerfError(f"{what}: expected None or a cell edge in lattice steps > 0, got {value!r}")
    value = float(value)
    if value == 0.0:
        return None
    if not (value > 0.0 and np.isfinite(value)):
        raise L.GpnerfError(f"{what}: expected None or a cell edge in lattice steps > 0, got {value!r}")
    return value


def simplify_grid(vmin, vmax, cell):
    """The grid simplify_mesh lays over a mesh whose box it was not given: lo = float32(floor(min) - cell / 4), cells =
    ceil((max - lo) / cell) + 1 per axis, in float64 on the host from the float32 box (the quarter cell keeps vertices with integer
    coordinates -- marching cubes' -- off the cell planes when cell is an integer; the extra cell holds max when it lies on one)."""
    vmin, vmax = np.asarray(vmin, dtype=np.float64), np.asarray(vmax, dtype=np.float64)
    lo = (np.floor(vmin) - float(cell) / 4.0).astype(np.float32)
    cells = np.ceil((vmax - lo.astype(np.float64)) / float(cell)).astype(np.int64) + 1
    return lo, [int(c) for c in cells]


def simplify_mesh(vertices, faces, cell, lo=None, cells=None, want_map=False):
    """gpnerf_mesh_simplify_count + gpnerf_mesh_simplify_emit: quadric vertex clustering of a device mesh (vertices float32 [n,3], faces
    int32 [m,3]) over cubic cells of edge `cell` -- cubes in the vertices' units; for marching cubes' index units on the reference's
    cubic voxels that is geometric --: (vertices float32 [n',3], faces int32 [m',3], stats int64 [8] (_lib.SIMPLIFY_STATS names them),
    vertex_map int32 [n] or None), all on the device.  include/gpnerf_hip.h states the definition.
    lo (3 floats) and cells (3 ints, product <= 2^26): the grid; with either omitted the box comes from vertices.amin / amax, one
    more host read (24 bytes), by simplify_grid's rule -- a mesh with a vertex that is not finite needs the grid given.  The other
    host read is the two output sizes.  The workspace comes from torch's caching allocator per call and goes back when the call
    returns."""
    lib = L.lib()
    nv, nf = mesh_args(vertices, faces, "simplify_mesh")
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell) and np.float32(cell) > 0 and np.isfinite(np.float32(cell))):
        raise L.GpnerfError(f"simplify_mesh: cell must be > 0 and finite, got {cell!r}")
    dev = vertices.device
    if lo is None or cells is None:
        if nv == 0:
            lo, cells = np.zeros(3, dtype=np.float32), [1, 1, 1]
        else:
            box = torch.stack([vertices.amin(0), vertices.amax(0)]).cpu().numpy()
            if not np.isfinite(box).all():
                raise L.GpnerfError("simplify_mesh: a vertex is not finite; give lo and cells")
            lo, cells = simplify_grid(box[0], box[1], cell)
    lo = np.asarray(lo, dtype=np.float32).ravel()
    cells = [int(c) for c in np.asarray(cells).ravel()]
    if lo.shape != (3,) or len(cells) != 3 or not np.isfinite(lo).all():
        raise L.GpnerfError(f"simplify_mesh: lo is 3 finite floats and cells 3 integers, got {lo!r} and {cells!r}")
    if min(cells) < 1 or cells[0] * cells[1] * cells[2] > L.SIMPLIFY_MAX_CELLS:
        raise L.GpnerfError(f"simplify_mesh: cells {cells} refused (each >= 1, product <= 2^26): choose a larger cell")
    c_lo, c_cells = (C.c_float * 3)(*lo.tolist()), (C.c_int32 * 3)(*cells)
    nbytes = int(lib.gpnerf_mesh_simplify_workspace_bytes(nv, nf, c_cells))
    if nbytes <= 0:
        raise L.GpnerfError(f"simplify_mesh: sizes refused ({nv} vertices, {nf} faces, cells {cells})")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    stats = torch.empty((len(L.SIMPLIFY_STATS),), device=dev, dtype=torch.int64)
    st = _stream_ptr(dev)
    vp, fp = ptr(vertices), ptr(faces)
    L.check(lib.gpnerf_mesh_simplify_count(vp, nv, fp, nf, c_lo, cell, c_cells, ws.data_ptr(), ws.numel(), stats.data_ptr(), st),
            "gpnerf_mesh_simplify_count")
    n_out_v, n_out_f = (int(v) for v in stats[:2].cpu().tolist())
    out_v = torch.empty((n_out_v, 3), device=dev, dtype=torch.float32)
    out_f = torch.empty((n_out_f, 3), device=dev, dtype=torch.int32)
    vmap = torch.empty((nv,), device=dev, dtype=torch.int32) if want_map else None
    L.check(lib.gpnerf_mesh_simplify_emit(vp, nv, fp, nf, ws.data_ptr(), ws.numel(), n_out_v, n_out_f, ptr(out_v), ptr(out_f), ptr(vmap), st),
            "gpnerf_mesh_simplify_emit")
    return out_v, out_f, stats, vmap


def parse_smooth(value, what="smooth"):
    """extract_mesh(smooth=...) / Renderer(mesh_smooth=...) / GPNERF_MESH_SMOOTH -> None (off) or the number of Taubin iterations, an int
    in [1, 10 000]: off is None, False, 0, "0" or ""; anything else that is not such a whole number is refused."""
    if value is None or value is False:
        return None
    if isinstance(value, str):
        text = value.strip()
        if text in ("", "0"):
            return None
        try:
            value = int(text)
        except ValueError:
            raise L.GpnerfError(f"{what}: expected 0 or a number of iterations in [1, {L.SMOOTH_MAX_ITERATIONS}], got {text!r}") from None
    if isinstance(value, (float, np.floating)) and np.isfinite(value) and float(value) == int(value):
        value = int(value)
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise L.GpnerfError(f"{what}: expected None or a number of iterations in [1, {L.SMOOTH_MAX_ITERATIONS}], got {value!r}")
    value = int(value)
    if value == 0:
        return None
    if not 1 <= value <= L.SMOOTH_MAX_ITERATIONS:
        raise L.GpnerfError(f"{what}: expected None or a number of iterations in [1, {L.SMOOTH_MAX_ITERATIONS}], got {value!r}")
    return value


class MeshAdjacency:
    """gpnerf_mesh_adjacency's result, all on the device: `stats` int64 [10] (_lib.TOPOLOGY_STATS names them), and three views into
    `workspace`: `start` int64 [n_vertices + 1], `neighbours` int32 [6 n_faces] of which start[n_vertices] entries are in use (vertex
    v's unique neighbours in ascending index at start[v] .. start[v + 1]) and `vertex_flags` uint8 [n_vertices]
    (_lib.VERTEX_REFERENCED | _lib.VERTEX_BOUNDARY).  smooth_mesh takes it as `adjacency`."""

    def __init__(self, faces, n_vertices, workspace, stats, offsets):
        self.faces, self.n_vertices, self.n_faces, self.workspace, self.stats = faces, int(n_vertices), int(faces.shape[0]), workspace, stats
        self.start = view(workspace, offsets[L.ADJACENCY_START], 8 * (self.n_vertices + 1), torch.int64)
        self.neighbours = view(workspace, offsets[L.ADJACENCY_NEIGHBOURS], 24 * self.n_faces, torch.int32)
        self.vertex_flags = view(workspace, offsets[L.ADJACENCY_VERTEX_FLAGS], self.n_vertices, torch.uint8)


def _adjacency_faces(faces, n_vertices, what, device=None):
    rows3_arg(faces, what, "faces", torch.int32, device)
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, (int, np.integer)) or n_vertices < 0:
        raise L.GpnerfError(f"{what}: n_vertices must be an integer >= 0, got {n_vertices!r}")
    return int(n_vertices), int(faces.shape[0])


def mesh_adjacency(faces, n_vertices):
    """gpnerf_mesh_adjacency on device faces (int32 [m,3]) of a mesh of n_vertices vertices -> MeshAdjacency: the unique edges' classes
    counted, every vertex's unique neighbours in ascending index, the vertex flags.  include/gpnerf_hip.h states the definition.
    Nothing is read back; the workspace's size is a formula of the two counts."""
    lib = L.lib()
    nv, nf = _adjacency_faces(faces, n_vertices, "mesh_adjacency")
    nbytes = int(lib.gpnerf_mesh_adjacency_workspace_bytes(nv, nf))
    offsets = (C.c_int64 * 3)()
    if nbytes <= 0 or lib.gpnerf_mesh_adjacency_layout(nv, nf, offsets) != 0:
        raise L.GpnerfError(f"mesh_adjacency: sizes refused ({nv} vertices, {nf} faces; at most {L.ADJACENCY_MAX_FACES} faces)")
    dev = faces.device
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    stats = torch.empty((len(L.TOPOLOGY_STATS),), device=dev, dtype=torch.int64)
    L.check(lib.gpnerf_mesh_adjacency(ptr(faces), nf, nv, ws.data_ptr(), ws.numel(), stats.data_ptr(), _stream_ptr(dev)),
            "gpnerf_mesh_adjacency")
    return MeshAdjacency(faces, nv, ws, stats, [int(o) for o in offsets])


def mesh_topology(faces, n_vertices):
    """the topology counts of a device mesh: mesh_adjacency(faces, n_vertices).stats, device int64 [10]; read_mesh_topology names them"""
    return mesh_adjacency(faces, n_vertices).stats


def read_mesh_topology(stats):
    """mesh_topology's stats on the host (a tensor or array of 10) -> dict of the _lib.TOPOLOGY_STATS names, plus `closed` (no boundary
    and no non-manifold edge), `oriented` (no inconsistent and no non-manifold edge) and `watertight` (both).  Connected components and
    the genus: mesh_components / read_mesh_components."""
    res = row_dict(stats, L.TOPOLOGY_STATS, "read_mesh_topology")
    res["closed"] = res["boundary_edges"] == 0 and res["nonmanifold_edges"] == 0
    res["oriented"] = res["inconsistent_edges"] == 0 and res["nonmanifold_edges"] == 0
    res["watertight"] = res["closed"] and res["oriented"]
    return res


def smooth_mesh(vertices, faces=None, adjacency=None, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True):
    """gpnerf_mesh_smooth: Taubin's lambda | mu filter on a device mesh -> new device vertices float32 [n,3]; the faces are untouched.
    One iteration is a Jacobi pass with factor lam and one with factor mu over every vertex's unique neighbours, summed in float64 in
    ascending neighbour index (include/gpnerf_hip.h): the result does not depend on the order of the faces and is bit-reproducible.
    adjacency: a MeshAdjacency of this mesh to reuse; without one it is built from `faces` (int32 [m,3]).  pin_boundary (default): the
    vertices on a boundary or non-manifold edge stay where they are.  lam in (0, 1], mu in [-1, 0], iterations in [0, 10 000] (0: a
    copy).  Nothing is read back."""
    lib = L.lib()
    rows3_arg(vertices, "smooth_mesh", "vertices", torch.float32)
    nv = int(vertices.shape[0])
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= iterations <= L.SMOOTH_MAX_ITERATIONS:
        raise L.GpnerfError(f"smooth_mesh: iterations must be an integer in [0, {L.SMOOTH_MAX_ITERATIONS}], got {iterations!r}")
    lam, mu = float(lam), float(mu)
    if not (0.0 < lam <= 1.0) or not (-1.0 <= mu <= 0.0):
        raise L.GpnerfError(f"smooth_mesh: lam must be in (0, 1] and mu in [-1, 0], got {lam!r} and {mu!r}")
    if adjacency is None:
        if faces is None:
            raise L.GpnerfError("smooth_mesh: give faces or an adjacency")
        _adjacency_faces(faces, nv, "smooth_mesh", device=vertices.device)
        adjacency = mesh_adjacency(faces, nv)
    elif not isinstance(adjacency, MeshAdjacency) or adjacency.n_vertices != nv or adjacency.workspace.device != vertices.device:
        raise L.GpnerfError(f"smooth_mesh: adjacency must be a MeshAdjacency of a mesh of {nv} vertices on {vertices.device}")
    out = torch.empty_like(vertices)
    ws = adjacency.workspace
    L.check(lib.gpnerf_mesh_smooth(ptr(vertices), nv, ws.data_ptr(), ws.numel(), int(iterations), lam, mu,
                                   L.SMOOTH_PIN_BOUNDARY if pin_boundary else 0, ptr(out), _stream_ptr(vertices.device)),
            "gpnerf_mesh_smooth")
    return out


def parse_components(value, what="components"):
    """extract_mesh(components=...) / Renderer(mesh_components=...) / GPNERF_MESH_COMPONENTS -> None (off), "largest" (keep the component
    with the most faces) or a whole number N >= 1 (keep the components of at least N faces): off is None, False, 0, "0" or "";
    anything else is refused."""
    if value is None or value is False:
        return None
    if isinstance(value, str):
        text = value.strip()
        if text in ("", "0"):
            return None
        if text == "largest":
            return "largest"
        try:
            value = int(text)
        except ValueError:
            raise L.GpnerfError(f"{what}: expected 0, 'largest' or a number of faces >= 1, got {text!r}") from None
    if isinstance(value, (float, np.floating)) and np.isfinite(value) and float(value) == int(value):
        value = int(value)
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise L.GpnerfError(f"{what}: expected None, 'largest' or a number of faces >= 1, got {value!r}")
    value = int(value)
    if value == 0:
        return None
    if value < 1:
        raise L.GpnerfError(f"{what}: expected None, 'largest' or a number of faces >= 1, got {value!r}")
    return value


class MeshComponents:
    """gpnerf_mesh_components' result, all on the device: `stats` int64 [9] (_lib.COMPONENT_STATS names them), the MeshAdjacency it was
    built on (`adjacency`), and four views into `workspace`: `label` int32 [n_vertices] (the smallest vertex index of the vertex's
    component, -1 for a vertex no usable face references), `vertex_component` int32 [n_vertices] and `face_component` int32 [n_faces]
    (the component's number, components numbered in ascending label; -1 for an unreferenced vertex / an unusable face) and `table`
    int64 [n_vertices // 3, 6] (_lib.COMPONENT_COLS; only the first stats[0] rows are defined).  `keep` / `min_faces`: the selection
    the counts KEPT_* were made for; filter_components emits it."""

    def __init__(self, adjacency, workspace, stats, offsets, keep, min_faces):
        self.adjacency, self.workspace, self.stats, self.keep, self.min_faces = adjacency, workspace, stats, keep, min_faces
        self.n_vertices, self.n_faces = adjacency.n_vertices, adjacency.n_faces
        self.label = view(workspace, offsets[L.COMPONENTS_LABEL], 4 * self.n_vertices, torch.int32)
        self.vertex_component = view(workspace, offsets[L.COMPONENTS_VERTEX_COMPONENT], 4 * self.n_vertices, torch.int32)
        self.face_component = view(workspace, offsets[L.COMPONENTS_FACE_COMPONENT], 4 * self.n_faces, torch.int32)
        rows = self.n_vertices // 3
        self.table = view(workspace, offsets[L.COMPONENTS_TABLE], 8 * len(L.COMPONENT_COLS) * rows, torch.int64).view(rows, len(L.COMPONENT_COLS))


def _components_keep(keep, min_faces, what):
    """(keep, min_faces) as the wrappers take them -> the C call's (mode, min_faces): keep is None or "all", "largest", or a whole
    number N >= 1 (the components of at least N faces, which min_faces=N says too)"""
    if isinstance(keep, str) and keep == "all":
        keep = None
    keep = parse_components(keep, f"{what}: keep")
    if min_faces is not None:
        if keep is not None:
            raise L.GpnerfError(f"{what}: give keep or min_faces, not both")
        if isinstance(min_faces, bool) or not isinstance(min_faces, (int, np.integer)) or min_faces < 1:
            raise L.GpnerfError(f"{what}: min_faces must be an integer >= 1, got {min_faces!r}")
        keep = int(min_faces)
    if keep is None:
        return L.COMPONENTS_KEEP_ALL, 0
    if keep == "largest":
        return L.COMPONENTS_KEEP_LARGEST, 0
    return L.COMPONENTS_KEEP_MIN_FACES, keep


def mesh_components(faces, n_vertices, adjacency=None, keep=None, min_faces=None):
    """gpnerf_mesh_components on device faces (int32 [m,3]) of a mesh of n_vertices vertices -> MeshComponents: the connected components
    of the graph of the usable faces' edges (VERTEX connectivity: two sheets that touch in one vertex are one component, where
    trimesh.split's default, face adjacency, gives two), labelled, numbered in ascending label, with their table and the stats.
    include/gpnerf_hip.h states the definition.  adjacency: a MeshAdjacency of this mesh to reuse; without one it is built here.
    keep: None or "all" (every component), "largest", or N (the components of at least N faces; min_faces=N says the same) -- it
    decides the stats' KEPT_* counts and what filter_components emits from this result.  Nothing is read back; the workspace's size is
    a formula of the two counts."""
    lib = L.lib()
    nv, nf = _adjacency_faces(faces, n_vertices, "mesh_components")
    mode, n_min = _components_keep(keep, min_faces, "mesh_components")
    if adjacency is None:
        adjacency = mesh_adjacency(faces, nv)
    elif not isinstance(adjacency, MeshAdjacency) or adjacency.n_vertices != nv or adjacency.n_faces != nf or adjacency.workspace.device != faces.device:
        raise L.GpnerfError(f"mesh_components: adjacency must be a MeshAdjacency of a mesh of {nv} vertices and {nf} faces on {faces.device}")
    nbytes = int(lib.gpnerf_mesh_components_workspace_bytes(nv, nf))
    offsets = (C.c_int64 * 4)()
    if nbytes <= 0 or lib.gpnerf_mesh_components_layout(nv, nf, offsets) != 0:
        raise L.GpnerfError(f"mesh_components: sizes refused ({nv} vertices, {nf} faces; at most {L.ADJACENCY_MAX_FACES} faces)")
    dev = faces.device
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    stats = torch.empty((len(L.COMPONENT_STATS),), device=dev, dtype=torch.int64)
    aws = adjacency.workspace
    L.check(lib.gpnerf_mesh_components(ptr(faces), nf, nv, aws.data_ptr(), aws.numel(), mode, n_min, ws.data_ptr(),
                                       ws.numel(), stats.data_ptr(), _stream_ptr(dev)), "gpnerf_mesh_components")
    return MeshComponents(adjacency, ws, stats, [int(o) for o in offsets], mode, n_min)


def read_mesh_components(stats, table=None, topology_stats=None):
    """mesh_components' stats on the host (a tensor or array of 9) -> dict of the _lib.COMPONENT_STATS names.  With `table` (the
    MeshComponents' table or its first rows) `rows` is added: one dict per component with the _lib.COMPONENT_COLS names, `closed`
    (boundary_vertices == 0) and `genus`: (2 - euler) // 2 when the component is closed, the mesh's inconsistent_edges and
    nonmanifold_edges are both 0 -- `topology_stats`, the adjacency's stats, says so; without it no genus is given -- and euler is
    even; None otherwise.  `largest_genus` is that of the largest component (None when there is none or no table).  A PINCHED vertex --
    all of its edges manifold, but its link more than one cycle (two cones tip to tip) -- is NOT detected: it leaves every count this
    rule reads as a closed manifold's would be, and makes the genus wrong."""
    res = row_dict(stats, L.COMPONENT_STATS, "read_mesh_components")
    if table is None:
        return res
    tab = host_int64(table)
    if tab.ndim != 2 or tab.shape[1] != len(L.COMPONENT_COLS) or tab.shape[0] < res["components"]:
        raise L.GpnerfError(f"read_mesh_components: expected a table of at least {res['components']} rows of {len(L.COMPONENT_COLS)}, got {tab.shape}")
    manifold = False
    if topology_stats is not None:
        topo = read_mesh_topology(topology_stats)
        manifold = topo["inconsistent_edges"] == 0 and topo["nonmanifold_edges"] == 0
    rows = []
    for r in tab[:res["components"]]:
        d = {k: int(v) for k, v in zip(L.COMPONENT_COLS, r)}
        d["closed"] = d["boundary_vertices"] == 0
        d["genus"] = (2 - d["euler"]) // 2 if d["closed"] and manifold and d["euler"] % 2 == 0 else None
        rows.append(d)
    res["rows"] = rows
    res["largest_genus"] = rows[res["largest"]]["genus"] if res["largest"] >= 0 else None
    return res


def filter_components(vertices, faces, keep="largest", components=None, want_map=False):
    """gpnerf_mesh_components + gpnerf_mesh_components_emit: the device mesh (vertices float32 [n,3], faces int32 [m,3]) of the kept
    components -> (vertices float32 [n',3], faces int32 [m',3], stats int64 [9] (_lib.COMPONENT_STATS), maps), all on the device.  keep:
    "largest" (default), N (the components of at least N faces) or None / "all" (every component: only the unreferenced vertices and
    the unusable faces go).  The kept vertices and faces stay in their original order, the coordinates are copied bit for bit.
    components: a MeshComponents of this mesh to emit from (its own keep decides; `keep` is then not looked at).  want_map: maps =
    (vertex_map int32 [n], old -> new or -1; kept_vertices int32 [n'], new -> old: attribute.index_select(0, kept_vertices.long())
    carries a per-vertex attribute over), otherwise None.  One host read: the two kept sizes."""
    lib = L.lib()
    nv, nf = mesh_args(vertices, faces, "filter_components")
    if components is None:
        components = mesh_components(faces, nv, keep=keep)
    elif not isinstance(components, MeshComponents) or components.n_vertices != nv or components.n_faces != nf or components.workspace.device != vertices.device:
        raise L.GpnerfError(f"filter_components: components must be a MeshComponents of a mesh of {nv} vertices and {nf} faces on {vertices.device}")
    dev = vertices.device
    n_out_v, n_out_f = (int(v) for v in components.stats[len(L.COMPONENT_STATS) - 2:].cpu().tolist())
    out_v = torch.empty((n_out_v, 3), device=dev, dtype=torch.float32)
    out_f = torch.empty((n_out_f, 3), device=dev, dtype=torch.int32)
    vmap = torch.empty((nv,), device=dev, dtype=torch.int32) if want_map else None
    kept = torch.empty((n_out_v,), device=dev, dtype=torch.int32) if want_map else None
    ws = components.workspace
    L.check(lib.gpnerf_mesh_components_emit(ptr(vertices), nv, ptr(faces), nf, ws.data_ptr(), ws.numel(), n_out_v, n_out_f, ptr(out_v), ptr(out_f),
                                            ptr(vmap), ptr(kept), _stream_ptr(dev)), "gpnerf_mesh_components_emit")
    return out_v, out_f, components.stats, ((vmap, kept) if want_map else None)


def _repair_flags(weld, drop_duplicates, orient, outward):
    if outward and not orient:
        raise L.GpnerfError("repair_mesh: outward needs orient (a patch is turned outward as a whole, behind its faces' common winding)")
    return ((L.REPAIR_WELD if weld else 0) | (L.REPAIR_DROP_DUPLICATES if drop_duplicates else 0) | (L.REPAIR_ORIENT if orient else 0) |
            (L.REPAIR_OUTWARD if outward else 0))


def repair_mesh(vertices, faces, tol=0.0, weld=True, drop_duplicates=True, orient=True, outward=True, want_map=False):
    """gpnerf_mesh_repair + gpnerf_mesh_repair_emit: a loaded device mesh (vertices float32 [n,3], faces int32 [m,3]: a triangle soup, a
    merged export with repeated faces and mixed windings, an inside-out scan) made fit for the mesh tools here -> (vertices float32
    [n',3], faces int32 [m',3], stats int64 [16] (_lib.REPAIR_STATS; read_mesh_repair names them)), all on the device.  include/
    gpnerf_hip.h states the definition.  weld: the vertices of one key become the lowest index among them -- tol == 0: equal float32
    coordinates, -0.0 as +0.0; tol > 0: the same cell of the grid of step tol (CELL clustering: two vertices closer than tol either side
    of a cell wall stay apart); drop_duplicates: of the faces on one set of three vertices the lowest index stays; orient: every
    edge-connected patch gets one winding (the minority flips); outward: a closed patch is turned to enclose positive volume (each by
    itself: a cavity's wall ends up facing its own outside -- leave outward off to keep it).  Faces with an index out of range, a
    non-finite corner or two equal corners and the vertices no face uses are always dropped; a kept vertex keeps its coordinates bit
    for bit, and vertices and faces stay in their original order.  want_map: a fourth result, a namespace of vertex_map int32 [n]
    (old -> new, following the weld; -1 dropped), kept_vertices int32 [n'] (new -> old), face_map int32 [m'] (new -> old), face_fate
    uint8 [m] (_lib.REPAIR_FATES) and face_patch int32 [m'] (the lowest original face index of the face's patch).  One host read: the
    two output sizes."""
    lib = L.lib()
    nv, nf = mesh_args(vertices, faces, "repair_mesh")
    flags = _repair_flags(weld, drop_duplicates, orient, outward)
    tol = float(tol)
    if not (0.0 <= tol < float("inf")):
        raise L.GpnerfError(f"repair_mesh: tol must be finite and >= 0, got {tol!r}")
    nbytes = int(lib.gpnerf_mesh_repair_workspace_bytes(nv, nf))
    if nbytes <= 0:
        raise L.GpnerfError(f"repair_mesh: sizes refused ({nv} vertices, {nf} faces; at most {L.REPAIR_MAX_VERTICES} vertices and {L.ADJACENCY_MAX_FACES} faces)")
    dev = vertices.device
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    stats = torch.empty((len(L.REPAIR_STATS),), device=dev, dtype=torch.int64)
    L.check(lib.gpnerf_mesh_repair(ptr(vertices), nv, ptr(faces), nf, tol, flags, ws.data_ptr(), ws.numel(), stats.data_ptr(), _stream_ptr(dev)),
            "gpnerf_mesh_repair")
    n_out_v, n_out_f = (int(v) for v in stats[:2].cpu().tolist())
    out_v = torch.empty((n_out_v, 3), device=dev, dtype=torch.float32)
    out_f = torch.empty((n_out_f, 3), device=dev, dtype=torch.int32)
    maps = None
    if want_map:
        new = lambda n, dt: torch.empty((n,), device=dev, dtype=dt)
        maps = SimpleNamespace(vertex_map=new(nv, torch.int32), kept_vertices=new(n_out_v, torch.int32), face_map=new(n_out_f, torch.int32),
                               face_fate=new(nf, torch.uint8), face_patch=new(n_out_f, torch.int32))
    m = maps if maps is not None else SimpleNamespace(vertex_map=None, kept_vertices=None, face_map=None, face_fate=None, face_patch=None)
    L.check(lib.gpnerf_mesh_repair_emit(ptr(vertices), nv, ptr(faces), nf, ws.data_ptr(), ws.numel(), ptr(out_v), n_out_v, ptr(out_f), n_out_f,
                                        ptr(m.vertex_map), ptr(m.kept_vertices), ptr(m.face_map), ptr(m.face_fate), ptr(m.face_patch),
                                        _stream_ptr(dev)), "gpnerf_mesh_repair_emit")
    return (out_v, out_f, stats, maps) if want_map else (out_v, out_f, stats)


def read_mesh_repair(stats):
    """repair_mesh's stats on the host (a tensor or array of 16) -> dict of the _lib.REPAIR_STATS names, plus `changed`: True when
    anything was welded, dropped (a vertex or a face) or flipped -- False says the mesh came out as it went in."""
    res = row_dict(stats, L.REPAIR_STATS, "read_mesh_repair")
    res["changed"] = any(res[k] for k in ("vertices_welded", "vertices_unkeyable", "vertices_unreferenced", "faces_invalid", "faces_unkeyable",
                                          "faces_collapsed", "faces_duplicate", "faces_flipped"))
    return res


def repair_mesh_object(mesh, device=None, **kw):
    """repair_mesh on a mesh.Mesh -> (mesh.Mesh, stats dict of read_mesh_repair): the mesh is uploaded (float32 vertices), repaired with
    repair_mesh's keywords and read back.  vertex_colors are carried through kept_vertices (a welded group keeps its representative's
    colour); texture and face_uvs through face_map, the UV rows of a flipped face swapped like its corners.  vertex_normals are
    DROPPED: welding and flipping leave them stale (frame.mesh_normals or a fresh estimate replaces them)."""
    from .mesh import Mesh
    dev = torch.device(device if device is not None else "cuda:0")
    v, f = mesh_to_device(mesh, dev)
    out_v, out_f, stats, maps = repair_mesh(v, f, want_map=True, **kw)
    kept, face_map = maps.kept_vertices.cpu().numpy().astype(np.int64), maps.face_map.cpu().numpy().astype(np.int64)
    colours = None if getattr(mesh, "vertex_colors", None) is None else mesh.vertex_colors[kept]
    texture = uvs = None
    if getattr(mesh, "face_uvs", None) is not None:
        flipped = maps.face_fate.cpu().numpy()[face_map] == L.REPAIR_FATES.index("kept_flipped")
        uvs = mesh.face_uvs[face_map].copy()
        uvs[flipped] = uvs[flipped][:, [0, 2, 1]]
        texture = mesh.texture.copy()
    return Mesh(out_v.cpu().numpy(), out_f.cpu().numpy(), colours, None, texture, uvs), read_mesh_repair(stats)
