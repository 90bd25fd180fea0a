"""Device plumbing and argument checks shared by frame.py and the mesh tool modules (mesh_edit, mesh_query, mesh_lattice, mesh_draw).

In: what a caller handed a wrapper.  Out: the same objects, accepted -- or a GpnerfError whose text starts with the wrapper's name.
Every check runs before the wrapper allocates or enqueues anything.  Nothing here launches a kernel, and nothing here imports frame."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_WORKSPACES = {}


def _workspace(dev, nbytes):
    """The scratch a gpnerf_render_fused call borrows (tile queues, chained lists, the colour list: 0.5 GB for 512 x 512 x 64, 2 GB for
    1024 x 1024 x 64).  One tensor per (device, stream), kept and grown rather than allocated per call: the call owns it only until the
    stream reaches its end, and calls on one stream are ordered -- while a fresh torch.empty of that size per call can fall out of the
    caching allocator's pool and cost a device allocation (milliseconds of idle device) every frame."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(torch.cuda.current_stream(dev).cuda_stream))
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        _WORKSPACES.pop(key, None)
        ws = None               # (release the smaller one first)
        while len(_WORKSPACES) >= 4:        # (streams come and go: at most four are remembered)
            _WORKSPACES.pop(next(iter(_WORKSPACES)))
        ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        _WORKSPACES[key] = ws
    return ws


def _require_gpu(t, what):
    if not t.is_cuda:
        raise L.GpnerfError(f"{what} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")


def ptr(t):
    """the pointer a C entry point takes for an optional or possibly empty tensor: None (NULL) for None or no elements"""
    return t.data_ptr() if t is not None and t.numel() else None


def view(workspace, off, nbytes, dtype):
    """`nbytes` of a uint8 workspace from byte `off` on, seen as `dtype`"""
    return workspace[off:off + nbytes].view(dtype)


def _shape_text(want):
    return "[" + ",".join("..." if w is Ellipsis else "n" if w is None else str(w) for w in want) + "]"


def tensor_arg(t, what, dtype, shape=None, device=None, like=None):
    """THE argument check of the wrappers: `t` is a contiguous device tensor of `dtype` whose shape is `shape` (a tuple, None for a
    free axis, a leading Ellipsis for any leading axes; shape None: any), or `like`'s shape, on `device` if one is given.  Refused, in
    this order: what is no tensor, a CPU tensor, a wrong dtype, rank or shape, a non-contiguous tensor, another device.  what: the
    wrapper's name and the argument's, "simplify_mesh: vertices".  Returns t."""
    if not isinstance(t, torch.Tensor):
        raise L.GpnerfError(f"{what} must be a device tensor, got {type(t).__name__}")
    _require_gpu(t, what)
    if like is not None:
        shape = like.shape
    fits = True
    if shape is not None:
        have, want = t.shape, shape
        if want and want[0] is Ellipsis:            # any leading axes
            want = want[1:]
            have = have[max(len(have) - len(want), 0):]
        fits = len(have) == len(want)
        if fits:
            for s, w in zip(have, want):
                if w is not None and w != s:
                    fits = False
                    break
    if t.dtype != dtype or not fits or not t.is_contiguous():
        raise L.GpnerfError(f"{what}: expected a contiguous {dtype} tensor{' ' + _shape_text(shape) if shape is not None else ''}, got "
                            f"{t.dtype} {tuple(t.shape)}{'' if t.is_contiguous() else ', not contiguous'}")
    if device is not None and t.device != device:
        raise L.GpnerfError(f"{what} is on {t.device}, the call's other tensors on {device}: they are on different devices")
    return t


def rows3_arg(t, what, name, dtype, device=None, like=None):
    """tensor_arg(t, f"{what}: {name}", dtype, (None, 3), device, like) for the shape nearly every argument here has -- vertices,
    faces, points, normals: a valid one is accepted by one straight test, with no string built (three of these run in front of every
    point_mesh_distance launch); everything else goes to tensor_arg for its refusal.  name None: `what` already names the argument."""
    if (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype is dtype and t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous()
            and (device is None or t.device == device) and (like is None or t.shape == like.shape)):
        return t
    return tensor_arg(t, what if name is None else f"{what}: {name}", dtype, (None, 3), device, like)


def mesh_args(vertices, faces, what, min_faces=0):
    """a device mesh -- contiguous float32 vertices [n,3] and int32 faces [m,3], m >= min_faces, on one device: (n, m)"""
    rows3_arg(vertices, what, "vertices", torch.float32)
    rows3_arg(faces, what, "faces", torch.int32, vertices.device)
    nf = faces.shape[0]
    if nf < min_faces:
        raise L.GpnerfError(f"{what}: faces: expected int32 faces [m,3], m >= {min_faces}, got {tuple(faces.shape)}")
    return vertices.shape[0], nf


def mesh_to_device(mesh, device):
    """(vertices float32 [n,3], faces int32 [m,3]) on `device` from a mesh.Mesh, a (vertices, faces) pair of arrays or tensors"""
    v, f = (mesh.vertices, mesh.faces) if hasattr(mesh, "vertices") else mesh
    as_t = lambda a, dt: (a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=device, dtype=dt)
    return as_t(v, torch.float32).reshape(-1, 3).contiguous(), as_t(f, torch.int32).reshape(-1, 3).contiguous()


def _raster_mesh(vertices, faces, what, device=None):
    """a device mesh from (vertices, faces) device tensors, or -- faces None -- from a mesh.Mesh / a pair of host arrays, uploaded by
    mesh_to_device; unlike the distance entry points the rasteriser takes a mesh without faces"""
    if faces is None:
        pair = (vertices.vertices, vertices.faces) if hasattr(vertices, "vertices") else vertices
        if any(isinstance(t, torch.Tensor) for t in pair):
            for t, name in zip(pair, ("vertices", "faces")):
                if not isinstance(t, torch.Tensor):
                    raise L.GpnerfError(f"{what}: {name} must be a device tensor like the other")
                _require_gpu(t, f"{what}: {name}")
            device = pair[0].device
        vertices, faces = mesh_to_device(vertices, torch.device(device if device is not None else "cuda:0"))
    mesh_args(vertices, faces, what)
    return vertices, faces


def _points(t, what, like=None, device=None):
    return rows3_arg(t, what, None, torch.float32, device, like)


def _cube_dims(cube, what):
    tensor_arg(cube, f"{what}: cube", torch.float32, (None, None, None))
    return (C.c_int32 * 3)(*cube.shape)


def _raster_cams(Ks, RTs, what):
    host = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    cams = np.ascontiguousarray(np.concatenate([host(Ks).reshape(-1, 9), host(RTs).reshape(-1, 12)], axis=1))
    if not 1 <= cams.shape[0] <= L.RASTER_MAX_VIEWS:
        raise L.GpnerfError(f"{what}: 1 to {L.RASTER_MAX_VIEWS} cameras, got {cams.shape[0]}")
    return cams


def host_int64(a):
    """counts a caller read back or is about to (a tensor -- its copy is the read -- or an array) as an int64 numpy array"""
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a).astype(np.int64)


def row_dict(stats, names, what):
    """the head of the read_* functions: one row of counts (a tensor or array of len(names)) -> {name: int}"""
    row = host_int64(stats).reshape(-1)
    if row.shape != (len(names),):
        raise L.GpnerfError(f"{what}: expected {len(names)} counts, got {row.shape}")
    return {k: int(v) for k, v in zip(names, row)}
