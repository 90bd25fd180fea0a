"""A mesh or depth maps onto a lattice, and a lattice's cube back to a mesh (csrc/gpnerf_voxelize.hip, gpnerf_sdf.hip, gpnerf_fusion.hip,
gpnerf_mesh.hip's marching cubes).

In: a device mesh (contiguous float32 vertices [n,3], int32 faces [m,3]; or a mesh.Mesh / a pair alone, which is uploaded), or device
float32 depth maps [m,H,W] with their host cameras, and the lattice: lo, step, dims = (nx, ny, nz) POINTS at lo + (i, j, k) * step.
Out, on the device: packed solid occupancy (VoxelGrid: voxelize_mesh, voxelize_cube; voxel_stats compares two), a truncated signed
distance field (SdfGrid: mesh_sdf from a mesh, DepthFusion / fuse_depth from depth maps), and from a float32 cube [X,Y,Z] its
iso-surface (marching_cubes, which SdfGrid.offset_mesh runs on its own values -- so it lives here and not beside frame's other cube
tools).  The read_* functions name the counts on the host.  frame re-exports every public name."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._args import _cube_dims, _points, _raster_cams, _raster_mesh, _require_gpu, _stream_ptr, _workspace, host_int64, ptr, row_dict, tensor_arg


def marching_cubes(cube, iso=1.0 / 50.0):
    """gpnerf_mesh_count + gpnerf_mesh_emit on a device float32 cube [X,Y,Z]: (vertices float32 [nv,3], faces int32 [nf,3]), device.
    The two counts are the call's one device-to-host read (they size the outputs).  The workspace (8 bytes per cube point) is
    allocated per call from torch's caching allocator and released when the call returns."""
    lib = L.lib()
    dims = _cube_dims(cube, "marching_cubes")
    dev = cube.device
    nbytes = int(lib.gpnerf_mesh_workspace_bytes(dims))
    if nbytes <= 0:
        raise L.GpnerfError(f"marching_cubes: dims {tuple(cube.shape)} refused (each >= 2, at most 2^28 points)")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    counts = torch.empty((2,), device=dev, dtype=torch.int64)
    st = _stream_ptr(dev)
    L.check(lib.gpnerf_mesh_count(cube.data_ptr(), dims, float(iso), ws.data_ptr(), ws.numel(), counts.data_ptr(), st), "gpnerf_mesh_count")
    nv, nf = (int(v) for v in counts.cpu().tolist())
    verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
    faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)
    L.check(lib.gpnerf_mesh_emit(cube.data_ptr(), dims, float(iso), ws.data_ptr(), ws.numel(), nv, nf,
                                 ptr(verts), ptr(faces), st), "gpnerf_mesh_emit")
    return verts, faces


def _voxel_dims(dims, what):
    d = tuple(int(v) for v in dims)
    if len(d) != 3 or min(d) < 1 or d[0] * d[1] * d[2] > L.VOXEL_MAX_POINTS:
        raise L.GpnerfError(f"{what}: dims {d} refused (three entries, each >= 1, at most 2^28 points)")
    return d


def _voxel_lattice(lo, step, what):
    lat = np.concatenate([np.asarray(lo, np.float64).ravel(), np.asarray(step, np.float64).ravel()])
    if lat.shape != (6,) or not np.isfinite(lat).all() or not (lat[3:] > 0).all():
        raise L.GpnerfError(f"{what}: lo and step must be three finite numbers each, step > 0, got {lat.tolist()}")
    return np.ascontiguousarray(lat)


class VoxelGrid:
    """Packed solid occupancy on a lattice (the counterpart of the reference's libs/utils/voxels.py VoxelGrid, on lattice POINTS and on
    the device).  bits: device uint32 [nx,ny,ceil(nz/32)], point k of column (i, j) in bit k & 31 of word k >> 5; dims: (nx, ny, nz);
    lo, step: float64 [3], point (i, j, k) sits at lo + (i, j, k) * step; stats: voxelize_mesh's device int64 [6] (_lib.VOXEL_STATS)
    or None for a grid that came from a cube."""

    def __init__(self, bits, dims, lo=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), stats=None):
        self.bits, self.dims, self.stats = bits, _voxel_dims(dims, "VoxelGrid"), stats
        lat = _voxel_lattice(lo, step, "VoxelGrid")
        self.lo, self.step = lat[:3].copy(), lat[3:].copy()

    def _c_dims(self):
        return (C.c_int32 * 3)(*self.dims)

    @property
    def occupied(self):
        """the number of occupied points, device int64 [] (a view of stats where the grid has them; otherwise a popcount is enqueued)"""
        if self.stats is not None:
            return self.stats[L.VOXEL_STATS.index("occupied")]
        return voxel_stats(self)[L.VOXEL_A]

    @property
    def cell_volume(self):
        return float(self.step[0] * self.step[1] * self.step[2])

    def dense(self):
        """gpnerf_voxel_unpack: a device float32 cube [nx,ny,nz] of 0 / 1, which marching_cubes(iso=0.5) and cube_clean take"""
        cube = torch.empty(self.dims, device=self.bits.device, dtype=torch.float32)
        L.check(L.lib().gpnerf_voxel_unpack(self.bits.data_ptr(), self._c_dims(), cube.data_ptr(), _stream_ptr(self.bits.device)),
                "gpnerf_voxel_unpack")
        return cube

    def contains(self, points):
        """gpnerf_voxel_contains: device uint8 [n], 1 where the lattice point nearest to the point (device float32 [n,3]; rint per
        axis, half to even) is inside the dims and occupied; 0 for points outside or not finite"""
        pts = _points(points, "VoxelGrid.contains: points", device=self.bits.device)
        n = int(pts.shape[0])
        out = torch.empty((n,), device=self.bits.device, dtype=torch.uint8)
        lat = np.concatenate([self.lo, self.step])
        L.check(L.lib().gpnerf_voxel_contains(self.bits.data_ptr(), self._c_dims(), lat.ctypes.data_as(L.DP), ptr(pts), n, ptr(out),
                                              _stream_ptr(self.bits.device)), "gpnerf_voxel_contains")
        return out


def voxelize_mesh(vertices, faces, lo, step, dims, rule="parity"):
    """gpnerf_mesh_voxelize: the solid occupancy of a mesh on the lattice of dims = (nx, ny, nz) POINTS at lo + (i, j, k) * step, as a
    VoxelGrid (bits and stats on the device, nothing read back).  vertices, faces: device float32 [nv,3] and int32 [nf,3]; or
    faces=None and `vertices` a mesh.Mesh or a (vertices, faces) pair, which mesh_to_device uploads.  rule: "parity" (a point is
    inside when an odd number of faces lie above it in its column: independent of the faces' order and orientation) or "nonzero" (the
    signed count is not 0: overlapping closed parts unite).  include/gpnerf_hip.h states which face owns a column (half-open, exact)
    and where it crosses; stats[_lib.VOXEL_STATS.index("open_columns")] > 0 says that the surface is not closed.  The workspace is
    the per-stream scratch rasterize_mesh borrows."""
    lib = L.lib()
    if rule not in L.VOXEL_RULES:
        raise L.GpnerfError(f"voxelize_mesh: rule is 'parity' or 'nonzero', got {rule!r}")
    vertices, faces = _raster_mesh(vertices, faces, "voxelize_mesh")
    d = _voxel_dims(dims, "voxelize_mesh")
    lat = _voxel_lattice(lo, step, "voxelize_mesh")
    cd = (C.c_int32 * 3)(*d)
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    nbytes = int(lib.gpnerf_mesh_voxelize_workspace_bytes(nf, cd, L.VOXEL_RULES[rule]))
    if nbytes <= 0:
        raise L.GpnerfError(f"voxelize_mesh: refused ({nf} faces, dims {d})")
    ws = _workspace(dev, nbytes)
    bits = torch.empty((d[0], d[1], (d[2] + 31) // 32), device=dev, dtype=torch.int32)
    stats = torch.empty((len(L.VOXEL_STATS),), device=dev, dtype=torch.int64)
    L.check(lib.gpnerf_mesh_voxelize(ptr(vertices), nv, ptr(faces), nf, lat.ctypes.data_as(L.DP), cd, L.VOXEL_RULES[rule], ws.data_ptr(),
                                     ws.numel(), bits.data_ptr(), stats.data_ptr(), _stream_ptr(dev)), "gpnerf_mesh_voxelize")
    return VoxelGrid(bits, d, lat[:3], lat[3:], stats)


def voxelize_cube(cube, iso=1.0 / 50.0, lo=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0)):
    """gpnerf_voxel_from_cube: the VoxelGrid of cube > iso (device float32 [X,Y,Z]; the iso value as marching_cubes takes it).  lo, step:
    the lattice the grid is said to live on (index units by default, the frame of marching_cubes' vertices)."""
    dims = _cube_dims(cube, "voxelize_cube")
    d = _voxel_dims(cube.shape, "voxelize_cube")
    bits = torch.empty((d[0], d[1], (d[2] + 31) // 32), device=cube.device, dtype=torch.int32)
    L.check(L.lib().gpnerf_voxel_from_cube(cube.data_ptr(), dims, float(iso), bits.data_ptr(), _stream_ptr(cube.device)), "gpnerf_voxel_from_cube")
    return VoxelGrid(bits, d, lo, step)


def voxel_stats(a, b=None, out=None):
    """gpnerf_voxel_stats: device int64 [4] (_lib.VOXEL_A, _B, _BOTH, _EITHER: the occupied points of a, of b, of both, of either) of
    two VoxelGrids of the same dims; b None: B = BOTH = 0, EITHER = A.  out: an int64 [4] slot to write into.  Nothing is read back."""
    for g, name in ((a, "a"), (b, "b")):
        if g is None and name == "b":
            continue
        if not isinstance(g, VoxelGrid):
            raise L.GpnerfError(f"voxel_stats: {name} must be a VoxelGrid")
        _require_gpu(g.bits, f"voxel_stats: {name}")
    if b is not None and (b.dims != a.dims or b.bits.device != a.bits.device):
        raise L.GpnerfError(f"voxel_stats: the grids differ (dims {a.dims} on {a.bits.device}, {b.dims} on {b.bits.device})")
    dev = a.bits.device
    if out is None:
        out = torch.empty((L.VOXEL_COUNTS,), device=dev, dtype=torch.int64)
    L.check(L.lib().gpnerf_voxel_stats(a.bits.data_ptr(), b.bits.data_ptr() if b is not None else None, a._c_dims(), out.data_ptr(),
                                       _stream_ptr(dev)), "gpnerf_voxel_stats")
    return out


def read_volume_metrics(host_counts, step):
    """voxel_stats' counts on the host ([4], array or tensor) and the lattice's steps -> {"volume_a", "volume_b": count x the product
    of the steps, "iou" = both / either, "precision" = both / a, "recall" = both / b}; 0 / 0 is 1.0 (nothing where nothing is to be)."""
    c = host_int64(host_counts).reshape(L.VOXEL_COUNTS)
    cell = float(np.prod(np.asarray(step, np.float64).ravel()[:3]))
    ratio = lambda num, den: float(c[num]) / float(c[den]) if c[den] else 1.0
    return {"volume_a": float(c[L.VOXEL_A]) * cell, "volume_b": float(c[L.VOXEL_B]) * cell, "iou": ratio(L.VOXEL_BOTH, L.VOXEL_EITHER),
            "precision": ratio(L.VOXEL_BOTH, L.VOXEL_A), "recall": ratio(L.VOXEL_BOTH, L.VOXEL_B)}


class SdfGrid:
    """gpnerf_mesh_sdf's field with its lattice.  values: device float32 [nx,ny,nz], the distance to the mesh where it is within
    `band`, the band elsewhere, negative where the voxels' bit is set; face: device int32 of the same shape (the nearest face, -1
    beyond the band) or None; voxels: the VoxelGrid the signs came from, or None for the unsigned field; lo, step: float64 [3];
    dims; band: the float32 value the kernels compared against; stats: device int64 [8] (_lib.SDF_STATS)."""

    def __init__(self, values, face, voxels, lo, step, dims, band, stats):
        self.values, self.face, self.voxels, self.stats = values, face, voxels, stats
        self.dims, self.band = _voxel_dims(dims, "SdfGrid"), float(band)
        lat = _voxel_lattice(lo, step, "SdfGrid")
        self.lo, self.step = lat[:3].copy(), lat[3:].copy()

    def sample(self, points):
        """gpnerf_sdf_sample: the trilinear value of the field at device float32 points [n,3] -> device float32 [n]; NaN for a point
        that is not finite or lies outside the lattice.  Beyond the band the field is +-band, so the interpolant saturates there."""
        _require_gpu(self.values, "SdfGrid.sample: values")
        pts = _points(points, "SdfGrid.sample: points", device=self.values.device)
        if min(self.dims) < 2:
            raise L.GpnerfError(f"SdfGrid.sample: dims {self.dims} refused (each >= 2)")
        n, dev = int(pts.shape[0]), self.values.device
        out = torch.empty((n,), device=dev, dtype=torch.float32)
        lat = np.concatenate([self.lo, self.step])
        L.check(L.lib().gpnerf_sdf_sample(self.values.data_ptr(), (C.c_int32 * 3)(*self.dims), lat.ctypes.data_as(L.DP),
                                          ptr(pts), n, ptr(out), _stream_ptr(dev)), "gpnerf_sdf_sample")
        return out

    def offset_mesh(self, offset=0.0):
        """The surface sdf = offset -- the mesh grown (offset > 0) or shrunk (< 0) by that metric distance -- as (vertices float32
        [nv,3] in the lattice's frame, faces int32 [nf,3]), device: marching_cubes(-values, iso=-offset), which takes !(v < iso) as
        inside, with the vertices mapped by lo + v * step.  |offset| must be under the band: the field is flat beyond it."""
        offset = float(offset)
        if not abs(offset) < self.band:
            raise L.GpnerfError(f"SdfGrid.offset_mesh: |offset| = {abs(offset)} is not under the band {self.band}: the field is flat there")
        v, f = marching_cubes(-self.values, iso=-offset)
        lo, step = (torch.from_numpy(a).to(v.device) for a in (self.lo, self.step))
        return (lo + v.to(torch.float64) * step).to(torch.float32), f


def mesh_sdf(vertices, faces, lo, step, dims, band, rule="nonzero", voxels=None, want_face=False):
    """gpnerf_mesh_sdf: the truncated signed distance field of a mesh on the lattice of dims = (nx, ny, nz) POINTS at
    lo + (i, j, k) * step, as an SdfGrid (everything on the device, nothing read back).  vertices, faces: as voxelize_mesh takes them.
    band: metric, > 0, at most 1024 x the smallest step.  The sign is the lattice point's own occupancy: `voxels`, a VoxelGrid of the
    same lattice, or -- voxels None -- voxelize_mesh under `rule` ("nonzero" / "parity"); rule=None gives the unsigned field.
    include/gpnerf_hip.h states the definition: |value| and face equal point_mesh_distance(lattice points, max_dist=band) bit for
    bit, with inf read as the band."""
    lib = L.lib()
    d = _voxel_dims(dims, "mesh_sdf")
    lat = _voxel_lattice(lo, step, "mesh_sdf")
    band32 = float(np.float32(band))
    if not (np.isfinite(band32) and 0.0 < band32 <= L.SDF_MAX_BAND_STEPS * float(lat[3:].min())):
        raise L.GpnerfError(f"mesh_sdf: band {band} refused (finite, > 0, at most {L.SDF_MAX_BAND_STEPS} x the smallest step {float(lat[3:].min())})")
    vertices, faces = _raster_mesh(vertices, faces, "mesh_sdf")
    dev = vertices.device
    if voxels is not None:
        if not isinstance(voxels, VoxelGrid):
            raise L.GpnerfError("mesh_sdf: voxels must be a VoxelGrid")
        _require_gpu(voxels.bits, "mesh_sdf: voxels")
        if voxels.dims != d or voxels.bits.device != dev or not (np.array_equal(voxels.lo, lat[:3]) and np.array_equal(voxels.step, lat[3:])):
            raise L.GpnerfError(f"mesh_sdf: the voxels live on another lattice (dims {voxels.dims}, lo {voxels.lo.tolist()}, step "
                                f"{voxels.step.tolist()} on {voxels.bits.device})")
    elif rule is not None:
        if rule not in L.VOXEL_RULES:
            raise L.GpnerfError(f"mesh_sdf: rule is 'nonzero', 'parity' or None, got {rule!r}")
        voxels = voxelize_mesh(vertices, faces, lat[:3], lat[3:], d, rule=rule)
    cd = (C.c_int32 * 3)(*d)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    nbytes = int(lib.gpnerf_mesh_sdf_workspace_bytes(nf, cd))
    if nbytes <= 0:
        raise L.GpnerfError(f"mesh_sdf: refused ({nf} faces, dims {d})")
    ws = _workspace(dev, nbytes)                              # (the voxeliser's launches, if any, are in front of these on the stream)
    values = torch.empty(d, device=dev, dtype=torch.float32)
    face = torch.empty(d, device=dev, dtype=torch.int32) if want_face else None
    stats = torch.empty((len(L.SDF_STATS),), device=dev, dtype=torch.int64)
    L.check(lib.gpnerf_mesh_sdf(ptr(vertices), nv, ptr(faces), nf, lat.ctypes.data_as(L.DP), cd, band32,
                                voxels.bits.data_ptr() if voxels is not None else None, ws.data_ptr(), ws.numel(), values.data_ptr(),
                                face.data_ptr() if face is not None else None, stats.data_ptr(), _stream_ptr(dev)), "gpnerf_mesh_sdf")
    return SdfGrid(values, face, voxels, lat[:3], lat[3:], d, band32, stats)


def _fusion_band(band, lat, what):
    band32 = float(np.float32(band))
    if not (np.isfinite(band32) and 0.0 < band32 <= L.SDF_MAX_BAND_STEPS * float(lat[3:].min())):
        raise L.GpnerfError(f"{what}: band {band} refused (finite, > 0, at most {L.SDF_MAX_BAND_STEPS} x the smallest step {float(lat[3:].min())})")
    return band32


def _fusion_views(depth, Ks, RTs, weights, z_near, what, dev=None):
    """the checked (depth, weights, cams, n_views, H, W, z_near) of a fusion call"""
    tensor_arg(depth, f"{what}: depth", torch.float32, (None, None, None), device=dev)
    cams = _raster_cams(Ks, RTs, what)
    m = cams.shape[0]
    if depth.shape[0] != m:
        raise L.GpnerfError(f"{what}: {m} cameras, but depth {tuple(depth.shape)}: expected [{m},H,W]")
    H, W = int(depth.shape[1]), int(depth.shape[2])
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise L.GpnerfError(f"{what}: refused ({m} views, {H} x {W})")
    if weights is not None:
        tensor_arg(weights, f"{what}: weights", torch.float32, (m, H, W), device=depth.device)
    z_near = float(z_near)
    if not (np.isfinite(z_near) and z_near > 0.0):
        raise L.GpnerfError(f"{what}: z_near {z_near} refused (> 0 and finite)")
    return depth, weights, cams, m, H, W, z_near


class DepthFusion:
    """The running state of a depth-map fusion (gpnerf_fusion_integrate; include/gpnerf_hip.h states THE DEFINITION) on the lattice of
    dims = (nx, ny, nz) POINTS at lo + (i, j, k) * step: `sum` and `weight` device float64 [nx,ny,nz], `flags` device uint8 (bit 0:
    some view saw the point behind its surface; bit 1: some view saw it within the band of one).  band: metric, > 0, at most 1024 x the
    smallest step.  integrate() continues the sums, so any number of views goes through in groups of at most eight; grid() is the field
    so far.  17 bytes per lattice point; nothing is read back."""

    def __init__(self, lo, step, dims, band, device):
        self.dims = _voxel_dims(dims, "DepthFusion")
        lat = _voxel_lattice(lo, step, "DepthFusion")
        self.lo, self.step, self._lat = lat[:3].copy(), lat[3:].copy(), lat
        self.band = _fusion_band(band, lat, "DepthFusion")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.GpnerfError(f"DepthFusion: the state must live on the GPU (got {dev}); the HIP path has no CPU fallback")
        self.device = dev
        self.sum = torch.empty(self.dims, device=dev, dtype=torch.float64)
        self.weight = torch.empty(self.dims, device=dev, dtype=torch.float64)
        self.flags = torch.empty(self.dims, device=dev, dtype=torch.uint8)
        self.reset()

    def _c_dims(self):
        return (C.c_int32 * 3)(*self.dims)

    def reset(self):
        """gpnerf_fusion_reset: the state back to no view at all"""
        L.check(L.lib().gpnerf_fusion_reset(self._c_dims(), self.sum.data_ptr(), self.weight.data_ptr(), self.flags.data_ptr(),
                                            _stream_ptr(self.device)), "gpnerf_fusion_reset")
        return self

    def integrate(self, depth, Ks, RTs, weights=None, z_near=1e-6, carve=True):
        """gpnerf_fusion_integrate: 1 to 8 more views into the state.  depth: device float32 [m,H,W], CAMERA Z (rasterize_mesh's
        depth; raycast_mesh's t along pixel_rays), +inf where the pixel sees nothing -- with carve, such a pixel empties the space
        along its ray; without, it says nothing.  NaN, 0 and negative depths say nothing.  Ks [m,3,3], RTs [m,3,4]: host arrays, used
        in float64, rasterize_mesh's cameras; weights: device float32 [m,H,W] or None (1).  Returns the call's device int64 [m,6]
        counts (_lib.FUSION_FATES: the lattice points of each view under their fate)."""
        depth, weights, cams, m, H, W, z_near = _fusion_views(depth, Ks, RTs, weights, z_near, "DepthFusion.integrate", self.device)
        stats = torch.empty((m, L.FUSION_N_FATES), device=self.device, dtype=torch.int64)
        L.check(L.lib().gpnerf_fusion_integrate(depth.data_ptr(), weights.data_ptr() if weights is not None else None, cams.ctypes.data_as(L.DP),
                                                m, H, W, self._lat.ctypes.data_as(L.DP), self._c_dims(), self.band, z_near, int(bool(carve)),
                                                self.sum.data_ptr(), self.weight.data_ptr(), self.flags.data_ptr(), stats.data_ptr(),
                                                _stream_ptr(self.device)), "gpnerf_fusion_integrate")
        return stats

    def grid(self):
        """gpnerf_fusion_finalise: the field so far as an SdfGrid (face None, voxels None) whose stats are the device int64 [4] totals
        (_lib.FUSION_TOTALS): sum / weight clamped to the band where a view weighed in, -band where none did and some view saw the
        point behind its surface, +band elsewhere.  offset_mesh(0) is the fused surface."""
        values = torch.empty(self.dims, device=self.device, dtype=torch.float32)
        totals = torch.empty((L.FUSION_N_TOTALS,), device=self.device, dtype=torch.int64)
        L.check(L.lib().gpnerf_fusion_finalise(self.sum.data_ptr(), self.weight.data_ptr(), self.flags.data_ptr(), self._c_dims(), self.band,
                                               values.data_ptr(), totals.data_ptr(), _stream_ptr(self.device)), "gpnerf_fusion_finalise")
        return SdfGrid(values, None, None, self.lo, self.step, self.dims, self.band, totals)


def fuse_depth(depth, Ks, RTs, lo, step, dims, band, weights=None, z_near=1e-6, carve=True, want_flags=False):
    """gpnerf_fusion_oneshot: at most eight depth maps fused into a truncated signed distance field in one pass -- what a fresh
    DepthFusion's integrate() and grid() give, bit for bit, with the sums in registers: 4 bytes written per lattice point instead of
    17 + 17 + 4 moved.  The arguments are DepthFusion's and integrate's.  Returns an SdfGrid (face None, voxels None, stats = the
    totals) with .fusion_stats (device int64 [m,6], _lib.FUSION_FATES), .fusion_totals (device int64 [4], _lib.FUSION_TOTALS) and, with
    want_flags, .flags (device uint8 [nx,ny,nz]) attached.  Nothing is read back."""
    d = _voxel_dims(dims, "fuse_depth")
    lat = _voxel_lattice(lo, step, "fuse_depth")
    band32 = _fusion_band(band, lat, "fuse_depth")
    depth, weights, cams, m, H, W, z_near = _fusion_views(depth, Ks, RTs, weights, z_near, "fuse_depth")
    dev = depth.device
    values = torch.empty(d, device=dev, dtype=torch.float32)
    flags = torch.empty(d, device=dev, dtype=torch.uint8) if want_flags else None
    stats = torch.empty((m, L.FUSION_N_FATES), device=dev, dtype=torch.int64)
    totals = torch.empty((L.FUSION_N_TOTALS,), device=dev, dtype=torch.int64)
    L.check(L.lib().gpnerf_fusion_oneshot(depth.data_ptr(), weights.data_ptr() if weights is not None else None, cams.ctypes.data_as(L.DP), m, H,
                                          W, lat.ctypes.data_as(L.DP), (C.c_int32 * 3)(*d), band32, z_near, int(bool(carve)), values.data_ptr(),
                                          flags.data_ptr() if flags is not None else None, stats.data_ptr(), totals.data_ptr(),
                                          _stream_ptr(dev)), "gpnerf_fusion_oneshot")
    grid = SdfGrid(values, None, None, lat[:3], lat[3:], d, band32, totals)
    grid.fusion_stats, grid.fusion_totals = stats, totals
    if want_flags:
        grid.flags = flags
    return grid


def read_fusion_stats(stats, totals):
    """fusion counts on the host (arrays or tensors; the one read, at the end) -> {"per_view": {name: [...]} for _lib.FUSION_FATES,
    **{name: count for _lib.FUSION_TOTALS}, "seen_fraction"}; stats may be several calls' rows stacked.  A fraction of nothing is 0."""
    s, named = host_int64(stats).reshape(-1, L.FUSION_N_FATES), row_dict(totals, L.FUSION_TOTALS, "read_fusion_stats")
    res = {"per_view": {name: [int(v) for v in s[:, k]] for k, name in enumerate(L.FUSION_FATES)}, **named}
    seen = named[L.FUSION_TOTALS[L.FUSION_SEEN]]
    n = seen + named[L.FUSION_TOTALS[L.FUSION_INTERIOR]] + named[L.FUSION_TOTALS[L.FUSION_UNKNOWN]]
    res["seen_fraction"] = float(seen) / n if n else 0.0
    return res
