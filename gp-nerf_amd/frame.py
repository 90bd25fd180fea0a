"""Per-frame constants and the Python face of the fused render entry point.

torch is used for device memory and streams only; all arithmetic of the path runs in
the HIP library (include/gpnerf_hip.h).  Nothing here falls back to PyTorch ops.
"""
import ctypes as C
from types import SimpleNamespace

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


def fetch_host(*items):
    """Small per-frame constants (camera matrices, Rh, Th, bounds, out_sh) as float64 numpy arrays with ONE device-to-host copy
    for all the device tensors among them (each `.cpu()` of its own is a synchronisation: six of them cost ~0.4 ms per frame)."""
    dev = [i for i, t in enumerate(items) if isinstance(t, torch.Tensor) and t.is_cuda]
    out = [None] * len(items)
    if dev:
        # float32 tensors travel as they are (the widening to float64 is exact and happens on the host: a cast per item on the
        # device was six launches per frame); anything else (int64 out_sh, float64 cameras) is widened on the device first
        f32 = [i for i in dev if items[i].dtype == torch.float32]
        rest = [i for i in dev if items[i].dtype != torch.float32]
        for group, widen in ((f32, False), (rest, True)):
            if not group:
                continue
            parts = [items[i].detach().reshape(-1) for i in group]
            if widen:
                parts = [p.to(torch.float64) for p in parts]
            cat = parts[0] if len(parts) == 1 else torch.cat(parts)
            flat = cat.cpu().numpy().astype(np.float64)
            pos = 0
            for i in group:
                n = items[i].numel()
                out[i] = flat[pos:pos + n].reshape(tuple(items[i].shape))
                pos += n
    for i, t in enumerate(items):
        if out[i] is None:
            out[i] = (t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)
    return out


def pack_head(state, device):
    """Pack the per-ray MLP parameters into the kernel's LDS image (gpnerf_pack_head).

    ``state`` maps reference parameter names (relative to ``nerfhead.``, e.g.
    ``rgbhead.base_fc.0.weight``) to tensors / arrays.  Returns a float32 device tensor.
    """
    lib = L.lib()
    params = L.GpnerfHeadParams()
    keep = []
    for short, name in L.HEAD_FIELDS:
        for suffix, field in (("weight", "_w"), ("bias", "_b")):
            v = state[f"{name}.{suffix}"]
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.float32)
            want = L.HEAD_SHAPES[short] if suffix == "weight" else (L.HEAD_SHAPES[short][0],)
            if tuple(a.shape) != want:
                raise L.GpnerfError(f"{name}.{suffix}: shape {a.shape}, expected {want}")
            keep.append(a)
            setattr(params, short + field, a.ctypes.data_as(L.FP))
    n = int(lib.gpnerf_head_blob_floats())
    blob = np.zeros(n, np.float32)
    L.check(lib.gpnerf_pack_head(C.byref(params), blob.ctypes.data_as(L.FP)), "gpnerf_pack_head")
    out = torch.from_numpy(blob).to(device)
    # the f16 hi/lo image for GPNERF_FLAG_SPLIT_F16 rides along as an attribute of the fp32 one
    ns = int(lib.gpnerf_head_blob_split_floats())
    sblob = np.zeros(ns, np.float32)
    L.check(lib.gpnerf_pack_head_split(C.byref(params), sblob.ctypes.data_as(L.FP)), "gpnerf_pack_head_split")
    out._gpnerf_split = torch.from_numpy(sblob).to(device)
    # ... and the reference-order image (GPNERF_FLAG_REF_ORDER; the form every render uses unless it asks for folded levels)
    rblob = np.zeros(n, np.float32)
    L.check(lib.gpnerf_pack_head_ref(C.byref(params), rblob.ctypes.data_as(L.FP)), "gpnerf_pack_head_ref")
    out._gpnerf_ref = torch.from_numpy(rblob).to(device)
    return out


class Frame:
    """Everything render_rays reads that does not depend on the ray (BaseRender.py:110-157),
    re-laid out channels-last on the device.  Built once per target view."""

    def __init__(self, src_imgs, featmaps, volumes, src_Ks, src_poses, Rh, Th, bounds_min, voxel_size, out_sh,
                 head_blob, consts=None, imgs4=None):
        """
        src_imgs   [V,3,H,W] in [-1,1] (batch['src_imgs'][0]); de-normalised here (BaseRender.py:231)
        featmaps   [V,32,h,w]           encoder output (BaseRender.py:222)
        volumes    4 x [1,32,D,H,W] or [32,D,H,W]   dense levels (SparseConvNet.py:111)
        src_Ks [V,3,3], src_poses [V,3,4], Rh [3,3], Th [1,3] or [3], bounds_min [3] (xyz), voxel_size [3], out_sh [3] (dhw)
        head_blob  device tensor from pack_head()
        consts     optional: what fetch_host(src_Ks, src_poses, Rh, Th, bounds_min, voxel_size, out_sh) returned earlier, so that
                   building the frame does not synchronise with the device (Renderer.render fetches them before it enqueues
                   the encoder, while the queue is still empty)
        imgs4      optional: relayout_images(src_imgs) done earlier (Renderer.render does it beside the encoder)
        """
        lib = L.lib()
        dev = src_imgs.device
        for t, w in ((src_imgs, "src_imgs"), (featmaps, "featmaps"), (head_blob, "head_blob")):
            _require_gpu(t, w)
        if src_imgs.shape[0] != L.VIEWS or featmaps.shape[0] != L.VIEWS or featmaps.shape[1] != L.CH:
            raise L.GpnerfError(f"the kernels are built for V={L.VIEWS} views x {L.CH} channels "
                                f"(rgb_fc's 96 inputs hard-wire it: trainhead.py:96,143); got {tuple(src_imgs.shape)}, {tuple(featmaps.shape)}")
        if len(volumes) != L.LEVELS:
            raise L.GpnerfError(f"expected {L.LEVELS} volume levels, got {len(volumes)}")
        st = _stream_ptr(dev)
        self.device = dev
        f = L.GpnerfFrame()
        V, _, H, W = src_imgs.shape
        src = src_imgs.contiguous().float()
        if imgs4 is not None and (tuple(imgs4.shape) != (V, H, W, 4) or imgs4.dtype != torch.float32 or imgs4.device != dev or not imgs4.is_contiguous()):
            raise L.GpnerfError(f"imgs4 must be relayout_images(src_imgs): float32 [{V},{H},{W},4] on {dev}")
        self.imgs = imgs4 if imgs4 is not None else relayout_images(src)
        fh, fw = featmaps.shape[-2:]
        if (featmaps.dtype == torch.float32 and not featmaps.is_contiguous()
                and featmaps.is_contiguous(memory_format=torch.channels_last)):
            fm = featmaps                       # physical [V,h,w,32] already (encoder.ResUNet on the GPU): no copy
            self.featmaps = featmaps.permute(0, 2, 3, 1)
        else:
            fm = featmaps.contiguous().float()
            self.featmaps = torch.empty((V, fh, fw, L.CH), device=dev, dtype=torch.float32)
            L.check(lib.gpnerf_relayout_featmaps(fm.data_ptr(), self.featmaps.data_ptr(), V, fh, fw, st), "gpnerf_relayout_featmaps")
        keep = [src, fm]
        self._set_volumes(f, volumes, keep)
        self._keep = keep  # sources stay alive until the re-layout kernels have run (stream order)
        f.featmaps, f.feat_h, f.feat_w = self.featmaps.data_ptr(), fh, fw
        f.imgs, f.img_h, f.img_w = self.imgs.data_ptr(), H, W
        # K4 @ P4 in fp32, as train_intrinsics.bmm(train_poses) does (BaseRender.py:233-247,314)
        Ks_h, poses_h, Rh_h, Th_h, bmin_h, vox_h, osh_h = consts if consts is not None else fetch_host(src_Ks, src_poses, Rh, Th, bounds_min,
                                                                                                          voxel_size, out_sh)
        KP = np.zeros((2, V, 4, 4), np.float32)
        KP[:, :, 3, 3] = 1.0
        KP[0, :, :3, :3] = Ks_h.astype(np.float32).reshape(V, 3, 3)
        KP[1, :, :3, :4] = poses_h.astype(np.float32).reshape(V, 3, 4)
        KPt = torch.from_numpy(KP)
        M = torch.bmm(KPt[0], KPt[1]).numpy()              # (torch's own CPU product: its multiply-add order is the reference's)
        for v in range(V):
            f.proj[v][:] = M[v].ravel()[:12].tolist()

        def flat(a, n):
            a = a.astype(np.float32).ravel()
            assert a.size == n, (a.shape, n)
            return a.tolist()

        f.Rh[:] = flat(Rh_h, 9)
        f.Th[:] = flat(Th_h, 3)
        f.bounds_min[:] = flat(bmin_h, 3)
        f.voxel[:] = flat(vox_h, 3)
        f.out_sh[:] = [int(v) for v in osh_h.ravel()[:3]]
        self.head_blob = head_blob
        f.head_blob = head_blob.data_ptr()
        self.head_blob_split = getattr(head_blob, "_gpnerf_split", None)
        f.head_blob_split = self.head_blob_split.data_ptr() if self.head_blob_split is not None else None
        self.head_blob_ref = getattr(head_blob, "_gpnerf_ref", None)
        f.head_blob_ref = self.head_blob_ref.data_ptr() if self.head_blob_ref is not None else None
        self.c = f

    def _set_volumes(self, f, volumes, keep):
        lib = L.lib()
        self.vols = []
        # whatever was derived from the previous levels goes with them: the folded coarse levels and the occupancy volume
        # would otherwise be read with the NEW levels' dimensions
        self._folded_valid, self.vols_folded, self.occ = False, None, None
        f.occ = None
        for l in range(L.LEVELS):
            f.vol_folded[l] = None
        for l, v in enumerate(volumes):
            _require_gpu(v, f"volumes[{l}]")
            if getattr(v, "_gpnerf_ndhwc", False):            # already channels-last (gpnerf_sparse_to_dense): no copy
                if v.shape[-1] != L.CH or v.dtype != torch.float32 or not v.is_contiguous():
                    raise L.GpnerfError(f"volume level {l}: expected contiguous fp32 [D,H,W,{L.CH}]")
                self.vols.append(v)
                f.vol[l] = v.data_ptr()
                f.vol_dhw[l][0], f.vol_dhw[l][1], f.vol_dhw[l][2] = v.shape[0], v.shape[1], v.shape[2]
                continue
            v = v.reshape(v.shape[-4:]).contiguous().float()
            if v.shape[0] != L.CH:
                raise L.GpnerfError(f"volume level {l}: {v.shape[0]} channels, expected {L.CH}")
            D, Hh, Ww = v.shape[1:]
            o = torch.empty((D, Hh, Ww, L.CH), device=v.device, dtype=torch.float32)
            L.check(lib.gpnerf_relayout_volume(v.data_ptr(), o.data_ptr(), D, Hh, Ww, _stream_ptr(v.device)),
                    "gpnerf_relayout_volume")
            self.vols.append(o)
            keep.append(v)
            f.vol[l] = o.data_ptr()
            f.vol_dhw[l][0], f.vol_dhw[l][1], f.vol_dhw[l][2] = D, Hh, Ww

    def build_occupancy(self):
        """SparseConvNet.encode's `masks3d` (SparseConvNet.py:135-139) from the 4 levels; enables occ_cull renders."""
        D, H, W = self.vols[0].shape[:3]
        self.occ = torch.empty((D, H, W), device=self.vols[0].device, dtype=torch.float32)
        L.check(L.lib().gpnerf_build_occupancy(C.byref(self.c), self.occ.data_ptr(), _stream_ptr(self.occ.device)),
                "gpnerf_build_occupancy")
        self.c.occ = self.occ.data_ptr()
        return self.occ

    def fold_volumes(self):
        """gpnerf_fold_volumes: the sigma feature layer applied to every voxel of the two coarse levels (64 values per voxel), so
        that the fp32 form interpolates their share of the layer's pre-activation instead of running it per sample.  Per-frame
        work (~10 us): the buffers are allocated once per Frame, every call recomputes them on the current stream."""
        if getattr(self, "vols_folded", None) is None:
            self.vols_folded = [torch.empty(tuple(v.shape[:3]) + (2 * L.CH,), device=v.device, dtype=torch.float32) if l >= L.FOLD_FIRST_LEVEL
                                else None for l, v in enumerate(self.vols)]
        ptrs = (C.c_void_p * L.LEVELS)(*[v.data_ptr() if v is not None else None for v in self.vols_folded])
        L.check(L.lib().gpnerf_fold_volumes(C.byref(self.c), ptrs, _stream_ptr(self.vols[0].device)), "gpnerf_fold_volumes")
        self._folded_valid = True
        return self.vols_folded

    @classmethod
    def for_volumes(cls, volumes, head_blob):
        """A frame that carries only the 4 dense levels (enough for gpnerf_sample_volume)."""
        if len(volumes) != L.LEVELS:
            raise L.GpnerfError(f"expected {L.LEVELS} volume levels, got {len(volumes)}")
        self = cls.__new__(cls)
        f = L.GpnerfFrame()
        self._keep = []
        self._set_volumes(f, volumes, self._keep)
        self.device = self.vols[0].device
        self.head_blob = head_blob
        f.head_blob = head_blob.data_ptr() if head_blob is not None else None
        self.c = f
        return self

    @staticmethod
    def consts_of_batch(batch, voxel_size):
        """The frame's small constants on the host, ONE device-to-host copy: Frame(..., consts=this)."""
        return fetch_host(batch["src_Ks"][0], batch["src_poses"][0], batch["Rh"][0], batch["Th"][0], batch["bounds"][0, 0], voxel_size,
                          batch["out_sh"][0])

    @classmethod
    def from_batch(cls, batch, featmaps, volumes, voxel_size, head_blob, consts=None, imgs4=None):
        """batch: the reference's batch dict (leading dim 1) with device tensors."""
        return cls(batch["src_imgs"][0], featmaps, volumes, batch["src_Ks"][0], batch["src_poses"][0], batch["Rh"][0],
                   batch["Th"][0], batch["bounds"][0, 0], voxel_size, batch["out_sh"][0], head_blob, consts=consts, imgs4=imgs4)


def relayout_images(src_imgs):
    """[V,3,H,W] in [-1,1] -> the frame's [V,H,W,4] image (de-normalised, channels-last, one padding channel: a pixel is one
    16-byte load), on the current stream (gpnerf_relayout_images)."""
    _require_gpu(src_imgs, "src_imgs")
    src = src_imgs.contiguous().float()
    V, _, H, W = src.shape
    out = torch.empty((V, H, W, 4), device=src.device, dtype=torch.float32)
    L.check(L.lib().gpnerf_relayout_images(src.data_ptr(), out.data_ptr(), V, H, W, _stream_ptr(src.device)), "gpnerf_relayout_images")
    return out


def patch_order(mask_at_box, H, W, patch_w=32, patch_h=8):
    """Permutation of the hit-ray list (raster order of `mask_at_box`) into image patches: each run of
    patch_w*patch_h consecutive slots covers one patch, one patch row (patch_w pixels) per wavefront.
    Returns an int32 numpy array for render_fused(ray_order=...)."""
    m = np.asarray(mask_at_box).reshape(H, W).astype(bool)
    idx = np.full((H, W), -1, np.int64)
    idx[m] = np.arange(int(m.sum()))
    Hp, Wp = -(-H // patch_h) * patch_h, -(-W // patch_w) * patch_w
    pad = np.full((Hp, Wp), -1, np.int64)
    pad[:H, :W] = idx
    t = pad.reshape(Hp // patch_h, patch_h, Wp // patch_w, patch_w).transpose(0, 2, 1, 3).reshape(-1)
    return t[t >= 0].astype(np.int32)


def patch_order_device(mask, H, W, patch_w=4, patch_h=8, n_kept=None):
    """patch_order() on the device for a bool mask [H*W]: int32 permutation that lays the kept pixels out patch by patch,
    so that a wavefront's 32 rays cover a compact patch_w x patch_h block instead of a 32-pixel row.  With sample culling a
    compact block is empty or full together far more often (measured: -10 % frame time at 10-30 % occupancy)."""
    m = mask.view(H, W)
    idx = (torch.cumsum(m.reshape(-1).to(torch.int32), 0, dtype=torch.int32) - 1).view(H, W)
    idx = torch.where(m, idx, torch.full_like(idx, -1))
    Hp, Wp = -(-H // patch_h) * patch_h, -(-W // patch_w) * patch_w
    if (Hp, Wp) != (H, W):
        idx = torch.nn.functional.pad(idx, (0, Wp - W, 0, Hp - H), value=-1)
    t = idx.view(Hp // patch_h, patch_h, Wp // patch_w, patch_w).permute(0, 2, 1, 3).reshape(-1)
    if n_kept is not None:
        # the caller knows how many pixels the mask keeps (it holds their rays): compaction with a static size, no host round trip
        # (boolean indexing synchronises to learn the count); a wrong n_kept shows up as -1 entries / a short list and is rejected
        pos = torch.nonzero_static(t >= 0, size=int(n_kept), fill_value=-1).squeeze(1)
        return t.index_select(0, pos.clamp_min(0)).masked_fill_(pos < 0, -1).contiguous()
    return t[t >= 0].contiguous()


def patch_order_rays(mask, H, W, n, patch_w=32, patch_h=8):
    """patch_order() for the n rays of a frame whose kept pixels are `mask` (bool / uint8 device tensor [H*W]): three launches, no
    host round trip (gpnerf_patch_order); the identity when the mask does not keep exactly n pixels."""
    _require_gpu(mask, "mask_at_box")
    m = mask.reshape(-1)
    m = (m if m.dtype in (torch.uint8, torch.bool) else (m != 0)).contiguous()
    if m.numel() != H * W:
        raise L.GpnerfError(f"mask has {m.numel()} entries for a {H}x{W} image")
    lib = L.lib()
    scratch = torch.empty((int(lib.gpnerf_patch_order_scratch_bytes(H, W, patch_w, patch_h)) // 4,), device=m.device, dtype=torch.int32)
    order = torch.empty((int(n),), device=m.device, dtype=torch.int32)
    L.check(lib.gpnerf_patch_order(m.data_ptr(), H, W, patch_w, patch_h, int(n), scratch.data_ptr(), order.data_ptr(), _stream_ptr(m.device)),
            "gpnerf_patch_order")
    return order


def _prepare_call(frame, N, S, want, neg_ray, early_term, ray_order, occ_cull, load_balance, split_f16, flip, subset, guard, fold,
                  reserve_cus, exits, workspace_cap, shared_device, touch=True):
    """What render_fused and render_plan derive from their keyword arguments, in one place: the flags word, the launch's ray count,
    the bytes of workspace lent, and the GPNERF_PLAN_* facts of the call.  touch=True (the render) also brings the frame into the
    state the flags ask for (occupancy volume built, coarse levels folded or not); touch=False only says what that state would be."""
    lib = L.lib()
    if flip is None:
        flip = bool(neg_ray) and not occ_cull
    flags = (L.FLAG_NEG_RAY if neg_ray else 0) | (L.FLAG_FLIP_SAMPLES if flip else 0) | (L.FLAG_EARLY_TERM if early_term else 0)
    flags |= (int(reserve_cus) & 0xff) << 24
    if not exits:
        flags |= L.FLAG_NO_EXITS
    if shared_device:
        flags |= L.FLAG_SHARED_DEVICE
    if split_f16:
        if frame is not None and not frame.c.head_blob_split:
            raise L.GpnerfError("split_f16 needs the f16 hi/lo head image (build the frame from pack_head()'s tensor)")
        flags |= L.FLAG_SPLIT_F16
        if guard is None:
            guard = bool(load_balance)
        if guard:
            if not load_balance:
                raise L.GpnerfError("the split form's range guard keeps its flags in the workspace (load_balance=True)")
            flags |= L.FLAG_SPLIT_GUARD
    if occ_cull:
        if touch and not frame.c.occ:
            frame.build_occupancy()
        flags |= L.FLAG_OCC_CULL
    if ray_order is not None:
        _require_gpu(ray_order, "ray_order")
        if ray_order.dtype != torch.int32 or not ray_order.is_contiguous() or (ray_order.numel() != N and not subset):
            raise L.GpnerfError("ray_order must be a contiguous int32 tensor with one entry per ray")
    n_launch = int(ray_order.numel()) if subset else N
    refold = fold is True
    fold = bool(fold)
    folded = fold and not split_f16
    if touch:
        if folded:
            if refold or not getattr(frame, "_folded_valid", False):
                frame.fold_volumes()
            for l in range(L.FOLD_FIRST_LEVEL, L.LEVELS):
                frame.c.vol_folded[l] = frame.vols_folded[l].data_ptr()
        else:
            for l in range(L.LEVELS):
                frame.c.vol_folded[l] = None
    if subset and any(k in want for k in ("weights", "z_vals", "raw")):
        raise L.GpnerfError("subset launches return the per-ray maps only")
    ws_bytes = int(lib.gpnerf_render_workspace_bytes(n_launch, S)) if load_balance else 0
    if workspace_cap is not None:       # lend less than the launch could use (it then keeps to the forms that fit: include/gpnerf_hip.h `workspace`)
        ws_bytes = min(ws_bytes, int(workspace_cap))
    facts = ((L.PLAN_WEIGHTS if "weights" in want else 0) | (L.PLAN_RAW if "raw" in want else 0) |
             (L.PLAN_SAMPLES_DONE if "samples_done" in want else 0) | (L.PLAN_FOLDED if folded else 0) |
             (L.PLAN_OCC if occ_cull or (frame is not None and frame.c.occ) else 0))
    return flags, n_launch, ws_bytes, facts


def render_plan(frame, rays, n_samples, neg_ray=False, early_term=False, term_eps=1e-5,
                want=("weights", "z_vals", "rgb_in", "ray_mask"), ray_order=None, occ_cull=False, load_balance=True,
                split_f16=False, flip=None, subset=False, guard=None, fold=None, reserve_cus=0, exits=True, workspace_cap=None, shared_device=False,
                n_cus=None):
    """What render_fused(frame, rays, n_samples, ...) with the same keyword arguments would launch: the GpnerfRenderPlan of
    gpnerf_render_plan (arithmetic, colour mode, launch shape, grid, workspace regions).  Host arithmetic only: nothing is launched
    and the frame is left as it is.  rays: the tensor, or just its row count; frame may be None (a frame's state only matters for
    occ_cull=False on a frame that already carries an occupancy volume).  fold=True is taken as folded volumes the render call
    accepts (include/gpnerf_hip.h GPNERF_PLAN_FOLDED: it ignores levels beyond 32-bit byte offsets).  n_cus: the device's compute units (default: the current
    device's)."""
    N = int(rays) if isinstance(rays, int) else int(rays.shape[0])
    flags, n_launch, ws_bytes, facts = _prepare_call(frame, N, int(n_samples), want, neg_ray=neg_ray, early_term=early_term, ray_order=ray_order,
                                                     occ_cull=occ_cull, load_balance=load_balance, split_f16=split_f16, flip=flip, subset=subset,
                                                     guard=guard, fold=fold, reserve_cus=reserve_cus, exits=exits, workspace_cap=workspace_cap,
                                                     shared_device=shared_device, touch=False)
    if n_cus is None:
        n_cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    plan = L.GpnerfRenderPlan()
    L.check(L.lib().gpnerf_render_plan(n_launch, int(n_samples), flags, int(n_cus), facts, ws_bytes, C.byref(plan)), "gpnerf_render_plan")
    return plan


def render_fused(frame, rays, n_samples, neg_ray=False, early_term=False, term_eps=1e-5,
                 want=("weights", "z_vals", "rgb_in", "ray_mask"), ray_order=None, occ_cull=False, load_balance=True,
                 split_f16=False, flip=None, subset=False, guard=None, fold=None, reserve_cus=0, exits=True, workspace_cap=None, shared_device=False):
    """gpnerf_render_fused over rays [N,8] (device).  Returns a dict of device tensors [N,...].
    neg_ray: the Projector's front test (h_z < 0).  flip: raw2outputs(neg=True); defaults to neg_ray for the dense renderer
    (BaseRender.py:86-88) and to False with occ_cull, because the progressive renderer's integral never flips
    (demo_render.py:329-344).
    ray_order: optional int32 device tensor [N], a permutation that groups rays into cache-friendly tiles.
    load_balance: lend the kernel a workspace: large frames run persistent workgroups on a tile queue, small frames split a
    tile's samples over several wavefronts.
    split_f16: dense layers on f16 MFMA with fp32 operands split into hi + lo (GPNERF_FLAG_SPLIT_F16).
    guard: with split_f16, check every MFMA operand against the f16 range and render the tiles that reach it again in the fp32
    form (GPNERF_FLAG_SPLIT_GUARD; default on whenever the kernel has a workspace).  want=("guard_tiles",) returns how many
    32-ray tiles that were (int32 tensor [1]).
    subset: ray_order lists the rows of `rays` to render (any number of distinct rows); outputs keep rays' row count, rows
    that are not listed come back zero.
    fold: which fp32 form.  False / None (default): the REFERENCE-ORDER form -- every dense layer accumulates as the reference's
    sgemm does (k ascending from zero, bias last, unscaled), x / 3 and the trilinear taps round as the reference's do: on trained
    parameters it sits at the op-for-op CPU oracle's distance from the reference.  True: the round-4 fast
    form -- coarse levels folded into the sigma feature layer per frame (Frame.fold_volumes), log2(e)-scaled layers: ~8 % faster layer for layer (the same time once both defer the colour branch),
    the same 1e-5 at initialisation scale, 5-10 x further from the reference on trained-like parameters.  "keep": True without
    re-folding a Frame that is already folded.
    shared_device=True: other processes' kernels share the device (GPNERF_FLAG_SHARED_DEVICE): no launch waits for its own workgroups.
    exits=False: every layer evaluated for every sample (GPNERF_FLAG_NO_EXITS).  By default the fp32 forms leave out what cannot
    change an output, bit for bit: the sigma feature layer of levels whose features are zero in all 32 samples of a step, and the
    colour branch of samples whose weight alpha * T is zero (the rest are listed and evaluated 32 at a time -- by a second launch
    over the whole frame's list where the workspace has room for it, out of a per-wavefront queue otherwise: the same bits),
    and everything behind the sample at which all 32 rays of a tile have a transmittance of exactly 0;
    want=("step_stats",) returns the 8 counters of GpnerfOutputs.step_stats (steps, empty-space steps, steps minus colour
    evaluations, opaque-tail steps, volume levels left out, colour evaluations, 0, 0).  A launch that returns `raw` keeps the
    colour branch in the step.
    reserve_cus: plan the launch for that many fewer compute units (multiple of 8), leaving them to kernels of other streams
    (GPNERF_FLAG_RESERVE_CUS).  The maps are those of a chip with that many fewer CUs."""
    lib = L.lib()
    _require_gpu(rays, "rays")
    rays = rays.contiguous().float()
    N, S = rays.shape[0], int(n_samples)
    dev = rays.device
    if subset:
        if ray_order is None:
            raise L.GpnerfError("subset=True needs ray_order (the rows to render)")
        alloc = torch.zeros
    else:
        alloc = torch.empty
    res = {
        "rgb_map": alloc((N, 3), device=dev), "depth_map": alloc((N,), device=dev),
        "acc_map": alloc((N,), device=dev), "disp_map": alloc((N,), device=dev),
    }
    o = L.GpnerfOutputs()
    o.rgb, o.depth, o.acc, o.disp = (res[k].data_ptr() for k in ("rgb_map", "depth_map", "acc_map", "disp_map"))
    if "weights" in want:
        res["weights"] = torch.empty((N, S), device=dev)
        o.weights = res["weights"].data_ptr()
    if "z_vals" in want:
        res["z_vals"] = torch.empty((N, S), device=dev)
        o.z_vals = res["z_vals"].data_ptr()
    if "rgb_in" in want:
        res["rgb_in_map"] = torch.empty((N, 9), device=dev)
        o.rgb_in = res["rgb_in_map"].data_ptr()
    if "ray_mask" in want:
        res["ray_mask"] = torch.empty((N,), device=dev, dtype=torch.uint8)
        o.ray_mask = res["ray_mask"].data_ptr()
    if "raw" in want:
        res["raw"] = torch.empty((N, S, 4), device=dev)
        o.raw = res["raw"].data_ptr()
    if "step_stats" in want:                               # include/gpnerf_hip.h GpnerfOutputs.step_stats: 8 counters
        res["step_stats"] = torch.zeros((8,), device=dev, dtype=torch.int32)
        o.step_stats = res["step_stats"].data_ptr()
    if "samples_done" in want:
        res["samples_done"] = torch.empty((N,), device=dev, dtype=torch.int32)
        o.samples_done = res["samples_done"].data_ptr()
    flags, n_launch, ws_bytes, facts = _prepare_call(frame, N, S, want, neg_ray=neg_ray, early_term=early_term, ray_order=ray_order, occ_cull=occ_cull,
                                                 load_balance=load_balance, split_f16=split_f16, flip=flip, subset=subset, guard=guard, fold=fold,
                                                 reserve_cus=reserve_cus, exits=exits, workspace_cap=workspace_cap, shared_device=shared_device)
    if N:       # the facts render_plan passes for this call are the pointers set above (an empty tensor has none; nothing is launched)
        assert facts & (L.PLAN_WEIGHTS | L.PLAN_RAW | L.PLAN_SAMPLES_DONE) == ((L.PLAN_WEIGHTS if o.weights else 0) | (L.PLAN_RAW if o.raw else 0) |
                                                                                (L.PLAN_SAMPLES_DONE if o.samples_done else 0))
        assert bool(facts & L.PLAN_FOLDED) == bool(frame.c.vol_folded[L.LEVELS - 1]) and (not flags & L.FLAG_OCC_CULL or bool(frame.c.occ))
    ws = _workspace(dev, ws_bytes) if ws_bytes else None
    L.check(lib.gpnerf_render_fused(C.byref(frame.c), rays.data_ptr(), n_launch, S, flags, float(term_eps),
                                    ray_order.data_ptr() if ray_order is not None else None, C.byref(o),
                                    ws.data_ptr() if ws is not None else None, ws_bytes, _stream_ptr(dev)), "gpnerf_render_fused")
    if "guard_tiles" in want:
        # the flag count is the first word of the guard block, which is the tail of the workspace (include/gpnerf_hip.h)
        if flags & L.FLAG_SPLIT_GUARD:
            off = ((ws_bytes - int(lib.gpnerf_render_guard_bytes(n_launch))) // 256) * 256
            res["guard_tiles"] = ws[off:off + 4].view(torch.int32).clone()
        else:
            res["guard_tiles"] = torch.zeros((1,), device=dev, dtype=torch.int32)
    return res


def _ref_image(head_blob):
    """the reference-order image riding on pack_head()'s tensor (what the stage entry points stage into LDS)"""
    ref = getattr(head_blob, "_gpnerf_ref", None)
    if ref is None:
        raise L.GpnerfError("head_blob must be pack_head()'s tensor (it carries the reference-order image)")
    return ref


def head_forward(head_blob, vol_feat, rgb_feat, mask):
    """gpnerf_head_forward: vol_feat [P,128], rgb_feat [P,V,35], mask [P,V] -> raw [P,4]."""
    lib = L.lib()
    for t, w in ((vol_feat, "vol_feat"), (rgb_feat, "rgb_feat"), (mask, "mask")):
        _require_gpu(t, w)
    vol_feat, rgb_feat, mask = vol_feat.contiguous().float(), rgb_feat.contiguous().float(), mask.contiguous().float()
    P = vol_feat.shape[0]
    raw = torch.empty((P, 4), device=vol_feat.device)
    L.check(lib.gpnerf_head_forward(_ref_image(head_blob).data_ptr(), vol_feat.data_ptr(), rgb_feat.data_ptr(), mask.data_ptr(), P,
                                    raw.data_ptr(), _stream_ptr(vol_feat.device)), "gpnerf_head_forward")
    return raw


def sigma_features(head_blob, vol_feat, rgb_feat):
    """gpnerf_sigma_features: vol_feat [P,128], rgb_feat [P,V,35] -> sigma_feat [P,64], globalfeat [P,134]
    (NeRFSigmaHead.test_forward after its volume sampling, trainhead.py:61-76)."""
    lib = L.lib()
    for t, w in ((vol_feat, "vol_feat"), (rgb_feat, "rgb_feat")):
        _require_gpu(t, w)
    vol_feat, rgb_feat = vol_feat.contiguous().float(), rgb_feat.contiguous().float()
    P = vol_feat.shape[0]
    sf = torch.empty((P, 64), device=vol_feat.device)
    gf = torch.empty((P, 134), device=vol_feat.device)
    L.check(lib.gpnerf_sigma_features(_ref_image(head_blob).data_ptr(), vol_feat.data_ptr(), rgb_feat.data_ptr(), P, sf.data_ptr(), gf.data_ptr(),
                                      _stream_ptr(vol_feat.device)), "gpnerf_sigma_features")
    return sf, gf


def rgb_head_forward(head_blob, sigma_feat, rgb_feat, mask):
    """gpnerf_rgb_head_forward: sigma_feat [P,64], rgb_feat [P,V,35], mask [P,V] -> raw [P,4] (NeRFRGBHead.forward, trainhead.py:118-145)."""
    lib = L.lib()
    for t, w in ((sigma_feat, "sigma_feat"), (rgb_feat, "rgb_feat"), (mask, "mask")):
        _require_gpu(t, w)
    sigma_feat, rgb_feat, mask = sigma_feat.contiguous().float(), rgb_feat.contiguous().float(), mask.contiguous().float()
    P = sigma_feat.shape[0]
    raw = torch.empty((P, 4), device=sigma_feat.device)
    L.check(lib.gpnerf_rgb_head_forward(_ref_image(head_blob).data_ptr(), sigma_feat.data_ptr(), rgb_feat.data_ptr(), mask.data_ptr(), P,
                                        raw.data_ptr(), _stream_ptr(sigma_feat.device)), "gpnerf_rgb_head_forward")
    return raw


def composite(raw, z_vals, nvalid=None, neg=False):
    """gpnerf_composite: Renderer.raw2outputs (BaseRender.py:75-107)."""
    lib = L.lib()
    _require_gpu(raw, "raw")
    raw, z_vals = raw.contiguous().float(), z_vals.contiguous().float()
    N, S = z_vals.shape
    dev = raw.device
    res = {"rgb_map": torch.empty((N, 3), device=dev), "depth_map": torch.empty((N,), device=dev),
           "acc_map": torch.empty((N,), device=dev), "disp_map": torch.empty((N,), device=dev),
           "weights": torch.empty((N, S), device=dev), "ray_mask": torch.zeros((N,), device=dev, dtype=torch.uint8)}
    o = L.GpnerfOutputs()
    o.rgb, o.depth, o.acc, o.disp = (res[k].data_ptr() for k in ("rgb_map", "depth_map", "acc_map", "disp_map"))
    o.weights, o.ray_mask = res["weights"].data_ptr(), res["ray_mask"].data_ptr()
    nv = nvalid.contiguous().float() if nvalid is not None else None
    L.check(lib.gpnerf_composite(raw.data_ptr(), z_vals.data_ptr(), nv.data_ptr() if nv is not None else None, N, S,
                                 int(bool(neg)), C.byref(o), _stream_ptr(dev)), "gpnerf_composite")
    return res


def make_rays(H, W, K, R, T, bounds, device):
    """gpnerf_make_rays: get_rays + get_near_far (data_utils.py:47-63,96-130) on the device, bit-exact against numpy's run.
    K, R, T are used in the dtype they come in (the dataset reads them as float64, ZjumocapDataset.py:360-380): the
    inverses are np.linalg.inv in that dtype, as get_rays takes them (:49-51,57).

    Returns (rays [n,8] packed in raster order of the hit pixels, mask_at_box [H*W] bool)."""
    lib = L.lib()
    K, R, T = np.asarray(K), np.asarray(R), np.asarray(T).reshape(3, 1)
    R_inv = np.linalg.inv(R)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    Kinv, Rinv, o = f64(np.linalg.inv(K)), f64(R_inv), f64((-R_inv @ T).ravel())
    b = np.ascontiguousarray(np.asarray(bounds, np.float32))
    rays = torch.empty((H * W, 8), device=device)
    hit = torch.empty((H * W,), device=device, dtype=torch.uint8)
    L.check(lib.gpnerf_make_rays(H, W, Kinv.ctypes.data_as(L.DP), Rinv.ctypes.data_as(L.DP), o.ctypes.data_as(L.DP),
                                 b.ctypes.data_as(L.FP), rays.data_ptr(), hit.data_ptr(), _stream_ptr(rays.device)),
            "gpnerf_make_rays")
    mask = hit.bool()
    return rays[mask], mask


def sample_points(frame, rays, n_samples):
    """gpnerf_sample_points: (pts [N,S,3], z_vals [N,S], grid_coords [N,S,3]) as BaseRender.py:35-73 computes them."""
    lib = L.lib()
    _require_gpu(rays, "rays")
    rays = rays.contiguous().float()
    N, S, dev = rays.shape[0], int(n_samples), rays.device
    pts, z, grid = torch.empty((N, S, 3), device=dev), torch.empty((N, S), device=dev), torch.empty((N, S, 3), device=dev)
    L.check(lib.gpnerf_sample_points(C.byref(frame.c), rays.data_ptr(), N, S, pts.data_ptr(), z.data_ptr(), grid.data_ptr(),
                                     _stream_ptr(dev)), "gpnerf_sample_points")
    return pts, z, grid


def sample_volume(frame, grid):
    """gpnerf_sample_volume: grid [P,3] (normalised xyz) -> [P,128] features of the 4 dense levels."""
    lib = L.lib()
    _require_gpu(grid, "grid")
    grid = grid.reshape(-1, 3).contiguous().float()
    P = grid.shape[0]
    out = torch.empty((P, 128), device=grid.device)
    L.check(lib.gpnerf_sample_volume(C.byref(frame.c), grid.data_ptr(), P, out.data_ptr(), _stream_ptr(grid.device)),
            "gpnerf_sample_volume")
    return out


def project_gather(frame, pts, neg_ray=False):
    """gpnerf_project_gather: pts [P,3] -> (rgb_feat [P,V,35], mask [P,V]) as Projector.compute does (BaseRender.py:326-363)."""
    lib = L.lib()
    _require_gpu(pts, "pts")
    pts = pts.reshape(-1, 3).contiguous().float()
    P = pts.shape[0]
    feat = torch.empty((P, L.VIEWS, 35), device=pts.device)
    mask = torch.empty((P, L.VIEWS), device=pts.device)
    L.check(lib.gpnerf_project_gather(C.byref(frame.c), pts.data_ptr(), P, int(bool(neg_ray)), feat.data_ptr(), mask.data_ptr(),
                                      _stream_ptr(pts.device)), "gpnerf_project_gather")
    return feat, mask


def select_rays(frame, target_K, target_pose, H, W, voxel_size, bounds_min, Rh, Th, neg_ray=False, threshold=0.1,
                target_K_inv=None, compact=True, host=None):
    """Progressive ray selection of the inference renderer (demo_render.py:166-247) on the device:
    occupied voxels -> marked pixels (gpnerf_select_pixels) -> rays with near/far (gpnerf_make_rays_demo).
    Returns (rays [n,8] in raster order of the kept pixels, mask_at_box [H*W] bool); with compact=False the rays of ALL H*W
    pixels (rows of pixels that are not kept are unspecified) and the mask, without any host synchronisation when `host` --
    fetch_host(target_K, target_pose, voxel_size, bounds_min, Rh, Th[, target_K_inv]) done earlier -- is handed in."""
    lib = L.lib()
    if not frame.c.occ:
        frame.build_occupancy()
    occ = frame.occ
    dev = occ.device
    items = [target_K, target_pose, voxel_size, bounds_min, Rh, Th] + ([target_K_inv] if target_K_inv is not None else [])
    host = [np.ascontiguousarray(a.astype(np.float32).ravel()) for a in (host if host is not None else fetch_host(*items))]
    f32 = lambda a, n: a[:n]
    K, pose = f32(host[0], 9), f32(host[1], 12)
    vox, bmin, rh, th = f32(host[2], 3), f32(host[3], 3), f32(host[4], 9), f32(host[5], 3)
    sel = torch.empty((H * W,), device=dev, dtype=torch.uint8)
    mm = torch.empty((6,), device=dev, dtype=torch.int32)
    D1, H1, W1 = occ.shape
    st = _stream_ptr(dev)
    p = lambda a: a.ctypes.data_as(L.FP)
    L.check(lib.gpnerf_select_pixels(occ.data_ptr(), D1, H1, W1, float(threshold), p(vox), p(bmin), p(rh), p(th), p(pose), p(K),
                                     H, W, sel.data_ptr(), mm.data_ptr(), st), "gpnerf_select_pixels")
    # batch["target_K_inv"] is what the reference multiplies by (demo_render.py:204; the dataset makes it with
    # np.linalg.inv on the float32 K, ZjumocapDataset.py:480); without it, do the same here
    Kinv = f32(host[6], 9) if target_K_inv is not None else np.ascontiguousarray(np.linalg.inv(K.reshape(3, 3)).astype(np.float32).ravel())
    rays = torch.empty((H * W, 8), device=dev)
    hit = torch.empty((H * W,), device=dev, dtype=torch.uint8)
    # the box of the occupied voxels stays on the device (mm): no host round trip between the two launches
    L.check(lib.gpnerf_make_rays_demo(H, W, p(Kinv), p(pose), None, mm.data_ptr(), int(bool(neg_ray)),
                                      sel.data_ptr(), rays.data_ptr(), hit.data_ptr(), st), "gpnerf_make_rays_demo")
    mask = hit.bool()
    return (rays[mask], mask) if compact else (rays, mask)


def patch_order_of(idx, W, patch_w=4, patch_h=8):
    """The kept pixels idx (int64, raster order) re-ordered patch by patch (patch_w x patch_h pixel blocks, row-major inside a
    block): one key computation and one device sort.  Returns int32 row indices for render_fused(ray_order=..., subset=True)."""
    y, x = idx // W, idx % W
    key = ((y // patch_h) * ((W + patch_w - 1) // patch_w) + x // patch_w) * (patch_w * patch_h) + (y % patch_h) * patch_w + x % patch_w
    return idx[torch.argsort(key)].to(torch.int32)


# ---- geometry mode of the inference renderer (demo_render.py:166-175,249-311,366-376: use_rgbhead False) ---------------------------
MESH_PAD = 10                 # np.pad(cube, 10) (:370)


def lattice_axis(lo, hi, step):
    """torch.range(lo, hi + step, step) as demo_render.py:249-263 calls it, on the host: lo, hi float32 scalars (can_bounds entries),
    step the float64 voxel size.  end = float32(hi) + float32(step), rounded to float32 (a float32 0-d tensor plus a Python/numpy
    scalar); size = floor((end - lo) / step) + 1 and value i = lo + i * step, both in float64, the values rounded to float32."""
    lo, step = np.float64(np.float32(lo)), np.float64(step)
    end = np.float64(np.float32(np.float32(hi) + np.float32(step)))
    n = int(np.floor((end - lo) / step)) + 1
    return (lo + np.arange(max(n, 0), dtype=np.float64) * step).astype(np.float32)


def mesh_box(frame, voxel_size, bounds_min, Rh, Th, threshold=0.1, host=None):
    """can_bounds (demo_render.py:166-175) of a frame with its occupancy volume: min / max over the world points of the level-1 voxels
    whose occupancy is above `threshold`, z widened by 0.05 (float32 arithmetic), as host float32 [2,3] -- the box's six values are
    this call's one device-to-host read (they size the lattice).  gpnerf_select_pixels computes them; its pixel marks (of a one-pixel
    image) are not used.  host: fetch_host(voxel_size, bounds_min, Rh, Th) done earlier, or None."""
    lib = L.lib()
    if not frame.c.occ:
        frame.build_occupancy()
    occ = frame.occ
    dev = occ.device
    host = host if host is not None else fetch_host(voxel_size, bounds_min, Rh, Th)
    vox, bmin, rh, th = [np.ascontiguousarray(np.asarray(a, dtype=np.float32).ravel()) for a in host]
    eye_pose = np.ascontiguousarray(np.eye(3, 4, dtype=np.float32).ravel())
    eye_k = np.ascontiguousarray(np.eye(3, dtype=np.float32).ravel())
    sel = torch.empty((1,), device=dev, dtype=torch.uint8)
    mm = torch.empty((6,), device=dev, dtype=torch.int32)
    D1, H1, W1 = occ.shape
    p = lambda a: a.ctypes.data_as(L.FP)
    L.check(lib.gpnerf_select_pixels(occ.data_ptr(), D1, H1, W1, float(threshold), p(vox), p(bmin), p(rh), p(th), p(eye_pose), p(eye_k),
                                     1, 1, sel.data_ptr(), mm.data_ptr(), _stream_ptr(dev)), "gpnerf_select_pixels")
    bits = mm.cpu().numpy()
    bits = np.where(bits >= 0, bits, bits ^ 0x7FFFFFFF).astype(np.int32)
    box = bits.view(np.float32).reshape(2, 3).copy()
    if not np.all(box[0] <= box[1]):
        raise L.GpnerfError(f"mesh extraction: no level-1 voxel has occupancy above {threshold} (the reference's min over no points fails too)")
    box[0, 2] = np.float32(box[0, 2] - np.float32(0.05))
    box[1, 2] = np.float32(box[1, 2] + np.float32(0.05))
    return box


def lattice_axes(box, voxel_size):
    """The three lattice axes of demo_render.py:249-263 (float32 host arrays)."""
    vs = np.asarray(voxel_size, dtype=np.float64).ravel()
    return [lattice_axis(box[0, a], box[1, a], vs[a]) for a in range(3)]


def dataset_lattice_axis(lo, hi, step):
    """np.arange(lo, hi + step, step) as ZjumocapDataset.py:397-402 calls it (lo, hi float32 entries of can_bounds, step the float64
    voxel size), followed by :404's astype(float32), on the host.  The source line's result depends on numpy's promotion rules; the
    arithmetic here is fixed to the reference era's (numpy < 2, value-based casting: a float32 array scalar plus a Python float is
    float64, where NEP 50 would round the stop to float32): lo = the float32 bound widened, stop = float64(hi) + step,
    n = ceil((stop - lo) / step), value i = lo + i * step in float64, rounded to float32."""
    lo, step = np.float64(np.float32(lo)), np.float64(step)
    stop = np.float64(np.float32(hi)) + step
    n = int(np.ceil((stop - lo) / step))
    return (lo + np.arange(max(n, 0), dtype=np.float64) * step).astype(np.float32)


def dataset_lattice_axes(can_bounds, voxel_size):
    """The three lattice axes of ZjumocapDataset.py:397-402 (float32 host arrays): dataset_lattice_axis() per axis of can_bounds
    [2,3].  batch['pts'] is their meshgrid ('ij', x slowest)."""
    box = np.asarray(can_bounds, dtype=np.float32).reshape(2, 3)
    vs = np.asarray(voxel_size, dtype=np.float64).ravel()
    return [dataset_lattice_axis(box[0, a], box[1, a], vs[a]) for a in range(3)]


def _axes_to(axes, dev):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev, non_blocking=False) for a in axes]


def visual_hull(axes, masks, Ks, RTs):
    """gpnerf_visual_hull: batch['inside'] (ZjumocapDataset.prepare_inside_pts) of the lattice `axes` (host float32 arrays,
    dataset_lattice_axes()) carved on the device.  masks: device uint8 [n,h,w], the views of inside_view in order (0, 1, and 100 on
    the border band); Ks [n,3,3] and RTs [n,3,4] (T in metres): host arrays, used in float64.  Returns (inside uint8 [X,Y,Z] holding
    the mask VALUES -- a border value is sticky and counts as inside --, n_inside int64 [1]), both on the device; nothing is read
    back."""
    lib = L.lib()
    _require_gpu(masks, "masks")
    if masks.dtype != torch.uint8 or masks.dim() != 3 or not masks.is_contiguous():
        raise L.GpnerfError(f"visual_hull: expected contiguous uint8 masks [n,h,w], got {masks.dtype} {tuple(masks.shape)}")
    n, mh, mw = masks.shape
    cams = np.concatenate([np.asarray(Ks, dtype=np.float64).reshape(-1, 9), np.asarray(RTs, dtype=np.float64).reshape(-1, 12)], axis=1)
    if cams.shape[0] != n:
        raise L.GpnerfError(f"visual_hull: {n} masks but {cams.shape[0]} cameras")
    cams = np.ascontiguousarray(cams)
    dev = masks.device
    ax = _axes_to(axes, dev)
    dims = (C.c_int32 * 3)(*[len(a) for a in axes])
    inside = torch.empty(tuple(len(a) for a in axes), device=dev, dtype=torch.uint8)
    n_inside = torch.empty((1,), device=dev, dtype=torch.int64)
    L.check(lib.gpnerf_visual_hull(ax[0].data_ptr(), ax[1].data_ptr(), ax[2].data_ptr(), dims, n, masks.data_ptr(), mh, mw,
                                   cams.ctypes.data_as(L.DP), inside.data_ptr(), n_inside.data_ptr(), _stream_ptr(dev)), "gpnerf_visual_hull")
    return inside, n_inside


def density_lattice(frame, axes, neg_ray=False, pad=MESH_PAD, inside=None):
    """gpnerf_density_lattice: the padded alpha cube [X+2p, Y+2p, Z+2p] (float32, device) of the lattice `axes` (host float32 arrays,
    lattice_axes()), and the device int64 count of kept (occupied) points.  With `inside` (device uint8 or bool [X,Y,Z]: visual_hull()'s
    output or batch['inside']) it is gpnerf_density_lattice_masked: the kept points are the non-zero ones, grid coordinates are the
    renderer's (the frame's voxel size), and no occupancy volume is built."""
    lib = L.lib()
    if frame.c.head_blob_ref is None:
        raise L.GpnerfError("density_lattice: the frame's head blob must be pack_head()'s tensor (it carries the reference-order image)")
    dims = (C.c_int32 * 3)(*[len(a) for a in axes])
    if inside is not None:
        _require_gpu(inside, "inside")
        if inside.dtype == torch.bool:
            inside = inside.view(torch.uint8)
        if inside.dtype != torch.uint8 or tuple(inside.shape) != tuple(len(a) for a in axes) or not inside.is_contiguous():
            raise L.GpnerfError(f"density_lattice: inside must be contiguous uint8 / bool {tuple(len(a) for a in axes)}, got "
                                f"{inside.dtype} {tuple(inside.shape)}")
        dev = inside.device
        ax = _axes_to(axes, dev)
        cube = torch.empty(tuple(len(a) + 2 * pad for a in axes), device=dev, dtype=torch.float32)
        n_kept = torch.empty((1,), device=dev, dtype=torch.int64)
        L.check(lib.gpnerf_density_lattice_masked(C.byref(frame.c), ax[0].data_ptr(), ax[1].data_ptr(), ax[2].data_ptr(), dims, int(pad),
                                                  int(bool(neg_ray)), inside.data_ptr(), cube.data_ptr(), n_kept.data_ptr(),
                                                  _stream_ptr(dev)), "gpnerf_density_lattice_masked")
        return cube, n_kept
    if not frame.c.occ:
        frame.build_occupancy()
    dev = frame.occ.device
    ax = _axes_to(axes, dev)
    cube = torch.empty(tuple(len(a) + 2 * pad for a in axes), device=dev, dtype=torch.float32)
    n_kept = torch.empty((1,), device=dev, dtype=torch.int64)
    L.check(lib.gpnerf_density_lattice(C.byref(frame.c), ax[0].data_ptr(), ax[1].data_ptr(), ax[2].data_ptr(), dims, int(pad),
                                       int(bool(neg_ray)), cube.data_ptr(), n_kept.data_ptr(), _stream_ptr(dev)), "gpnerf_density_lattice")
    # (the axis tensors may go out of scope here: the caching allocator hands their memory out again only in stream order, after
    # the launch that reads them)
    return cube, n_kept


def lattice_of(axes, voxel_size, pad=MESH_PAD):
    """query_points' `lattice` for the padded cube of `axes` (lattice_axes(box, voxel_size)): (lo [3] float64 = the float32 axis
    starts widened, step [3] float64 = the voxel size lattice_axis() multiplied by, pad)."""
    lo = np.array([np.float64(a[0]) if len(a) else 0.0 for a in axes], dtype=np.float64)
    return lo, np.asarray(voxel_size, dtype=np.float64).ravel()[:3].copy(), int(pad)


def query_points(frame, pts, neg_ray=False, occ_cull=False, want=("rgb", "sigma"), lattice=None):
    """gpnerf_query_points: the radiance field (NeRFHead.forward in the reference-order form) at pts [n,3] (device float32,
    contiguous): a dict of device tensors, "rgb" [n,3] and "sigma" [n] (views of the reference's `raw` layout [n,4], also returned
    as "raw") and, if wanted, "alpha" [n] (1 - exp(-sigma)).  Without "rgb" in `want` the colour branch is left out (raw's rgb
    columns are 0).  occ_cull: the progressive renderer's occupancy cull (GPNERF_FLAG_OCC_CULL: grid coordinates with the literal
    0.005, points whose occupancy interpolates to 0 get zeros).  lattice: (lo[3], step[3], pad) -- pts are then index units of
    the padded lattice cube (marching-cubes vertices), mapped on the device to lo + (v - pad) * step in float64."""
    lib = L.lib()
    _require_gpu(pts, "pts")
    if pts.dtype != torch.float32 or not pts.is_contiguous() or pts.dim() != 2 or pts.shape[1] != 3:
        raise L.GpnerfError(f"query_points: expected contiguous float32 points [n,3], got {pts.dtype} {tuple(pts.shape)}")
    unknown = set(want) - {"rgb", "sigma", "alpha", "raw"}
    if unknown:
        raise L.GpnerfError(f"query_points: unknown outputs {sorted(unknown)}")
    if frame.c.head_blob_ref is None:
        raise L.GpnerfError("query_points: the frame's head blob must be pack_head()'s tensor (it carries the reference-order image)")
    if occ_cull and not frame.c.occ:
        frame.build_occupancy()
    dev = pts.device
    n = pts.shape[0]
    raw = torch.empty((n, 4), device=dev, dtype=torch.float32)
    alpha = torch.empty((n,), device=dev, dtype=torch.float32) if "alpha" in want else None
    flags = (L.FLAG_NEG_RAY if neg_ray else 0) | (L.FLAG_OCC_CULL if occ_cull else 0) | (0 if "rgb" in want else L.FLAG_DENSITY_ONLY)
    lat = None
    if lattice is not None:
        lo, step, pad = lattice
        lat = (C.c_double * 7)(*[float(v) for v in np.asarray(lo, np.float64).ravel()[:3]],
                               *[float(v) for v in np.asarray(step, np.float64).ravel()[:3]], float(pad))
    L.check(lib.gpnerf_query_points(C.byref(frame.c), pts.data_ptr() if n else None, n, flags, lat,
                                    raw.data_ptr() if n else None, alpha.data_ptr() if alpha is not None and n else None,
                                    _stream_ptr(dev)), "gpnerf_query_points")
    res = {"raw": raw, "sigma": raw[:, 3]}
    if "rgb" in want:
        res["rgb"] = raw[:, :3]
    if alpha is not None:
        res["alpha"] = alpha
    return res


def marching_cubes(cube, iso=1.0 / 50.0):
    """gpnerf_mesh_count + gpnerf_mesh_emit on a device float32 cube [X,Y,Z]: (vertices float32 [nv,3], faces int32 [nf,3]), device.
    The two counts are the call's one device-to-host read (they size the outputs).  The workspace (8 bytes per cube point) is
    allocated per call from torch's caching allocator and released when the call returns."""
    lib = L.lib()
    _require_gpu(cube, "cube")
    if cube.dim() != 3 or cube.dtype != torch.float32 or not cube.is_contiguous():
        raise L.GpnerfError("marching_cubes: expected a contiguous float32 [X,Y,Z] cube")
    dev = cube.device
    dims = (C.c_int32 * 3)(*cube.shape)
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
                                 verts.data_ptr() if nv else None, faces.data_ptr() if nf else None, st), "gpnerf_mesh_emit")
    return verts, faces


def _cube_dims(cube, what):
    _require_gpu(cube, "cube")
    if cube.dim() != 3 or cube.dtype != torch.float32 or not cube.is_contiguous():
        raise L.GpnerfError(f"{what}: expected a contiguous float32 [X,Y,Z] cube")
    return (C.c_int32 * 3)(*cube.shape)


def parse_keep(keep):
    """cube_clean's `keep` -> (flags, min_points): None keeps every component, "largest" the largest one, an integer N >= 1 those of
    at least N points."""
    if keep is None:
        return 0, 0
    if isinstance(keep, str):
        if keep != "largest":
            raise L.GpnerfError(f"cube_clean: keep is None, 'largest' or a number of points, got {keep!r}")
        return L.CUBE_KEEP, 0
    if isinstance(keep, bool) or int(keep) != keep or int(keep) < 1:
        raise L.GpnerfError(f"cube_clean: keep is None, 'largest' or a number of points >= 1, got {keep!r}")
    return L.CUBE_KEEP, int(keep)


def cube_clean(cube, iso=1.0 / 50.0, keep=None, fill_cavities=False, want_labels=False):
    """gpnerf_cube_clean on a device float32 cube [X,Y,Z]: (out_cube, stats, labels or None), all on the device, nothing read back.
    keep: None (every solid component stays), "largest", or N (components of at least N points stay); the inside points of the others
    become 0.  fill_cavities: below-iso regions that reach no face of the cube (6-connectivity), after that step, become 1.  stats:
    int64 [6], _lib.CUBE_STATS names them; labels: int32 [X,Y,Z], the lowest linear index of each inside point's 18-connected
    component, -1 elsewhere.  The workspace (8 bytes per point) comes from torch's caching allocator and goes back when the call
    returns."""
    lib = L.lib()
    dims = _cube_dims(cube, "cube_clean")
    flags, min_points = parse_keep(keep)
    flags |= L.CUBE_FILL if fill_cavities else 0
    nbytes = int(lib.gpnerf_cube_clean_workspace_bytes(dims))
    if nbytes <= 0:
        raise L.GpnerfError(f"cube_clean: dims {tuple(cube.shape)} refused (each >= 2, at most 2^28 points)")
    dev = cube.device
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    out = torch.empty_like(cube)
    stats = torch.empty((6,), device=dev, dtype=torch.int64)
    labels = torch.empty(tuple(cube.shape), device=dev, dtype=torch.int32) if want_labels else None
    L.check(lib.gpnerf_cube_clean(cube.data_ptr(), dims, float(iso), flags, min_points, ws.data_ptr(), ws.numel(), out.data_ptr(),
                                  labels.data_ptr() if labels is not None else None, stats.data_ptr(), _stream_ptr(dev)), "gpnerf_cube_clean")
    return out, stats, labels


def mesh_normals(cube, vertices, step=None):
    """gpnerf_mesh_normals: unit normals (device float32 [n,3]) at `vertices` (device float32 [n,3], index units of `cube`, e.g.
    marching_cubes' as they come) from the cube's central differences, pointing toward lower values.  step: the lattice's voxel size
    per axis (1 / step scales the differences, so that an anisotropic lattice gives geometric normals), or None for 1, 1, 1."""
    lib = L.lib()
    dims = _cube_dims(cube, "mesh_normals")
    _require_gpu(vertices, "vertices")
    if vertices.dtype != torch.float32 or not vertices.is_contiguous() or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise L.GpnerfError(f"mesh_normals: expected contiguous float32 vertices [n,3], got {vertices.dtype} {tuple(vertices.shape)}")
    n = vertices.shape[0]
    normals = torch.empty((n, 3), device=cube.device, dtype=torch.float32)
    inv = None
    if step is not None:
        inv = (C.c_float * 3)(*[float(np.float32(1.0) / np.float32(v)) for v in np.asarray(step, dtype=np.float64).ravel()[:3]])
    L.check(lib.gpnerf_mesh_normals(cube.data_ptr(), dims, vertices.data_ptr() if n else None, n, inv,
                                    normals.data_ptr() if n else None, _stream_ptr(cube.device)), "gpnerf_mesh_normals")
    return normals


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
    for t, name in ((vertices, "vertices"), (faces, "faces")):
        if not isinstance(t, torch.Tensor):
            raise L.GpnerfError(f"simplify_mesh: {name} must be a device tensor (mesh_to_device uploads a Mesh)")
        _require_gpu(t, f"simplify_mesh: {name}")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_contiguous():
        raise L.GpnerfError(f"simplify_mesh: expected contiguous float32 vertices [n,3], got {vertices.dtype} {tuple(vertices.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous():
        raise L.GpnerfError(f"simplify_mesh: expected contiguous int32 faces [m,3], got {faces.dtype} {tuple(faces.shape)}")
    if faces.device != vertices.device:
        raise L.GpnerfError("simplify_mesh: vertices and faces are on different devices")
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell) and np.float32(cell) > 0 and np.isfinite(np.float32(cell))):
        raise L.GpnerfError(f"simplify_mesh: cell must be > 0 and finite, got {cell!r}")
    dev = vertices.device
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
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
    vp, fp = (vertices.data_ptr() if nv else None), (faces.data_ptr() if nf else None)
    L.check(lib.gpnerf_mesh_simplify_count(vp, nv, fp, nf, c_lo, cell, c_cells, ws.data_ptr(), ws.numel(), stats.data_ptr(), st),
            "gpnerf_mesh_simplify_count")
    n_out_v, n_out_f = (int(v) for v in stats[:2].cpu().tolist())
    out_v = torch.empty((n_out_v, 3), device=dev, dtype=torch.float32)
    out_f = torch.empty((n_out_f, 3), device=dev, dtype=torch.int32)
    vmap = torch.empty((nv,), device=dev, dtype=torch.int32) if want_map else None
    L.check(lib.gpnerf_mesh_simplify_emit(vp, nv, fp, nf, ws.data_ptr(), ws.numel(), n_out_v, n_out_f, out_v.data_ptr() if n_out_v else None,
                                          out_f.data_ptr() if n_out_f else None, vmap.data_ptr() if vmap is not None and nv else None, st),
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
        view = lambda off, nbytes, dt: workspace[off:off + nbytes].view(dt)
        self.start = view(offsets[L.ADJACENCY_START], 8 * (self.n_vertices + 1), torch.int64)
        self.neighbours = view(offsets[L.ADJACENCY_NEIGHBOURS], 24 * self.n_faces, torch.int32)
        self.vertex_flags = view(offsets[L.ADJACENCY_VERTEX_FLAGS], self.n_vertices, torch.uint8)


def _adjacency_faces(faces, n_vertices, what):
    if not isinstance(faces, torch.Tensor):
        raise L.GpnerfError(f"{what}: faces must be a device tensor (mesh_to_device uploads a Mesh)")
    _require_gpu(faces, f"{what}: faces")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous():
        raise L.GpnerfError(f"{what}: expected contiguous int32 faces [m,3], got {faces.dtype} {tuple(faces.shape)}")
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
    L.check(lib.gpnerf_mesh_adjacency(faces.data_ptr() if nf else None, nf, nv, ws.data_ptr(), ws.numel(), stats.data_ptr(), _stream_ptr(dev)),
            "gpnerf_mesh_adjacency")
    return MeshAdjacency(faces, nv, ws, stats, [int(o) for o in offsets])


def mesh_topology(faces, n_vertices):
    """the topology counts of a device mesh: mesh_adjacency(faces, n_vertices).stats, device int64 [10]; read_mesh_topology names them"""
    return mesh_adjacency(faces, n_vertices).stats


def read_mesh_topology(stats):
    """mesh_topology's stats on the host (a tensor or array of 10) -> dict of the _lib.TOPOLOGY_STATS names, plus `closed` (no boundary
    and no non-manifold edge), `oriented` (no inconsistent and no non-manifold edge) and `watertight` (both).  Connected components and
    the genus: mesh_components / read_mesh_components."""
    row = np.asarray(stats.detach().cpu() if isinstance(stats, torch.Tensor) else stats).astype(np.int64).reshape(-1)
    if row.shape != (len(L.TOPOLOGY_STATS),):
        raise L.GpnerfError(f"read_mesh_topology: expected {len(L.TOPOLOGY_STATS)} counts, got {row.shape}")
    res = {k: int(v) for k, v in zip(L.TOPOLOGY_STATS, row)}
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
    if not isinstance(vertices, torch.Tensor):
        raise L.GpnerfError("smooth_mesh: vertices must be a device tensor (mesh_to_device uploads a Mesh)")
    _require_gpu(vertices, "smooth_mesh: vertices")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_contiguous():
        raise L.GpnerfError(f"smooth_mesh: expected contiguous float32 vertices [n,3], got {vertices.dtype} {tuple(vertices.shape)}")
    nv = int(vertices.shape[0])
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= iterations <= L.SMOOTH_MAX_ITERATIONS:
        raise L.GpnerfError(f"smooth_mesh: iterations must be an integer in [0, {L.SMOOTH_MAX_ITERATIONS}], got {iterations!r}")
    lam, mu = float(lam), float(mu)
    if not (0.0 < lam <= 1.0) or not (-1.0 <= mu <= 0.0):
        raise L.GpnerfError(f"smooth_mesh: lam must be in (0, 1] and mu in [-1, 0], got {lam!r} and {mu!r}")
    if adjacency is None:
        if faces is None:
            raise L.GpnerfError("smooth_mesh: give faces or an adjacency")
        _adjacency_faces(faces, nv, "smooth_mesh")
        if faces.device != vertices.device:
            raise L.GpnerfError("smooth_mesh: vertices and faces are on different devices")
        adjacency = mesh_adjacency(faces, nv)
    elif not isinstance(adjacency, MeshAdjacency) or adjacency.n_vertices != nv or adjacency.workspace.device != vertices.device:
        raise L.GpnerfError(f"smooth_mesh: adjacency must be a MeshAdjacency of a mesh of {nv} vertices on {vertices.device}")
    out = torch.empty_like(vertices)
    ws = adjacency.workspace
    L.check(lib.gpnerf_mesh_smooth(vertices.data_ptr() if nv else None, nv, ws.data_ptr(), ws.numel(), int(iterations), lam, mu,
                                   L.SMOOTH_PIN_BOUNDARY if pin_boundary else 0, out.data_ptr() if nv else None, _stream_ptr(vertices.device)),
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
        view = lambda off, nbytes, dt: workspace[off:off + nbytes].view(dt)
        self.label = view(offsets[L.COMPONENTS_LABEL], 4 * self.n_vertices, torch.int32)
        self.vertex_component = view(offsets[L.COMPONENTS_VERTEX_COMPONENT], 4 * self.n_vertices, torch.int32)
        self.face_component = view(offsets[L.COMPONENTS_FACE_COMPONENT], 4 * self.n_faces, torch.int32)
        rows = self.n_vertices // 3
        self.table = view(offsets[L.COMPONENTS_TABLE], 8 * len(L.COMPONENT_COLS) * rows, torch.int64).view(rows, len(L.COMPONENT_COLS))


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
    L.check(lib.gpnerf_mesh_components(faces.data_ptr() if nf else None, nf, nv, aws.data_ptr(), aws.numel(), mode, n_min, ws.data_ptr(),
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
    host = lambda t: np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t).astype(np.int64)
    row = host(stats).reshape(-1)
    if row.shape != (len(L.COMPONENT_STATS),):
        raise L.GpnerfError(f"read_mesh_components: expected {len(L.COMPONENT_STATS)} counts, got {row.shape}")
    res = {k: int(v) for k, v in zip(L.COMPONENT_STATS, row)}
    if table is None:
        return res
    tab = host(table)
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
    nv, nf = _mesh_arrays(vertices, faces, "filter_components")
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
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
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
    nv, nf = _mesh_arrays(vertices, faces, "repair_mesh")
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
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
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
    row = np.asarray(stats.detach().cpu() if isinstance(stats, torch.Tensor) else stats).astype(np.int64).reshape(-1)
    if row.shape != (len(L.REPAIR_STATS),):
        raise L.GpnerfError(f"read_mesh_repair: expected {len(L.REPAIR_STATS)} counts, got {row.shape}")
    res = {k: int(v) for k, v in zip(L.REPAIR_STATS, row)}
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


def _mesh_arrays(vertices, faces, what):
    """a device mesh that may be empty: (n_vertices, n_faces)"""
    for t, name in ((vertices, "vertices"), (faces, "faces")):
        if not isinstance(t, torch.Tensor):
            raise L.GpnerfError(f"{what}: {name} must be a device tensor (mesh_to_device uploads a Mesh)")
        _require_gpu(t, f"{what}: {name}")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_contiguous():
        raise L.GpnerfError(f"{what}: expected contiguous float32 vertices [n,3], got {vertices.dtype} {tuple(vertices.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous():
        raise L.GpnerfError(f"{what}: expected contiguous int32 faces [m,3], got {faces.dtype} {tuple(faces.shape)}")
    if faces.device != vertices.device:
        raise L.GpnerfError(f"{what}: vertices and faces are on different devices")
    return int(vertices.shape[0]), int(faces.shape[0])


def extract_mesh(frame, voxel_size, bounds_min, Rh, Th, neg_ray=False, iso=1.0 / 50.0, host=None, clean=None, fill_cavities=None,
                 normals=False, lattice=None, simplify=None, smooth=None, topology=False, components=None):
    """The geometry mode of demo_render.py's render_rays (:166-175, 249-311, 366-376) on the device: the box of the occupied voxels,
    the lattice, the alpha cube and its marching-cubes mesh.  Two host reads: the box (6 values) and the mesh counts (2).
    Returns {"cube" (device [X+20,Y+20,Z+20]), "vertices", "faces" (device), "axes", "can_bounds", "n_kept" (device int64),
    "lattice" (lattice_of(axes): query_points at the vertices as they come)}.
    clean (cube_clean's `keep`: "largest" or N) and fill_cavities (None: filled whenever clean is given): marching cubes then runs on
    the cleaned cube -- "cube" stays the untouched one -- and "clean_stats" (device int64 [6]) is added; normals: "normals" (device
    [nv,3], mesh_normals of the cube the mesh was made from, scaled by 1 / voxel size) is added.  simplify: a number k > 0, the edge in
    lattice steps of the cubic cells of simplify_mesh, which runs behind marching cubes on the index-unit vertices with lo = (-1/2,
    -1/2, -1/2) and cells = ceil(dim / k) + 1 (for an integer k the lattice planes, on which marching-cubes vertices have two integer
    coordinates, never sit on a cell boundary); "vertices" and "faces" are then the simplified mesh, "normals" are taken at ITS
    vertices, "simplify_stats" (device int64 [8], _lib.SIMPLIFY_STATS) is added, and the call has one more host read (the two sizes).
    The cells are cubes in index units: geometric on cubic voxels, as the reference's are.  smooth: a number n > 0 of Taubin
    iterations (smooth_mesh at its defaults: lam 0.5, mu -0.53, open borders pinned), which run behind marching cubes and simplify and
    in front of the normals, which are then taken at the smoothed vertices; topology: the mesh's topology counts.  With either,
    "topology_stats" (device int64 [10], _lib.TOPOLOGY_STATS: of the mesh as returned -- smoothing moves no face) is added, the
    adjacency is built once, and no host read is added.  components ("largest" or N, parse_components): filter_components runs behind
    marching cubes and simplify and in front of smoothing, topology and normals -- the components that are not kept (all but the one
    with the most faces, or those of fewer than N faces) leave the mesh, so that smoothing, "topology_stats", normals and colours are
    of the mesh as returned --; "component_stats" (device int64 [9], _lib.COMPONENT_STATS: the counts of the mesh BEFORE the filter and
    what was kept) is added, and the call has one more host read (the two kept sizes).  It builds an adjacency of the unfiltered mesh;
    when smoothing or topology is also on, the adjacency is built a second time, on the filtered mesh.  With components off no launch
    and no host read is added.  With all seven off no further launch is enqueued.
    lattice: a ready (cube, axes, n_kept) -- the dense renderer's hull-carved cube (density_lattice(inside=...)) -- in place of the
    box, the lattice and the occupancy-culled cube; cleaning, marching cubes, normals and "lattice" are then the same code.  The box
    read does not happen and "can_bounds" is left out."""
    vs = host[0] if host is not None else voxel_size
    if lattice is not None:
        cube, axes, n_kept = lattice
        res = {"cube": cube, "axes": axes, "n_kept": n_kept, "lattice": lattice_of(axes, vs)}
    else:
        box = mesh_box(frame, voxel_size, bounds_min, Rh, Th, host=host)
        axes = lattice_axes(box, vs)
        cube, n_kept = density_lattice(frame, axes, neg_ray=neg_ray)
        res = {"cube": cube, "axes": axes, "can_bounds": box, "n_kept": n_kept, "lattice": lattice_of(axes, vs)}
    fill = (clean is not None) if fill_cavities is None else bool(fill_cavities)
    surface = cube
    if clean is not None or fill:
        surface, res["clean_stats"], _ = cube_clean(cube, iso, keep=clean, fill_cavities=fill)
    res["vertices"], res["faces"] = marching_cubes(surface, iso)
    k = parse_simplify(simplify, "extract_mesh: simplify")
    if k is not None:
        cells = [int(np.ceil(d / k)) + 1 for d in surface.shape]
        res["vertices"], res["faces"], res["simplify_stats"], _ = simplify_mesh(res["vertices"], res["faces"], k, lo=(-0.5, -0.5, -0.5),
                                                                                cells=cells)
    keep = parse_components(components, "extract_mesh: components")
    if keep is not None:
        res["vertices"], res["faces"], res["component_stats"], _ = filter_components(res["vertices"], res["faces"], keep=keep)
    n_smooth = parse_smooth(smooth, "extract_mesh: smooth")
    if n_smooth is not None or topology:
        adjacency = mesh_adjacency(res["faces"], int(res["vertices"].shape[0]))
        res["topology_stats"] = adjacency.stats
        if n_smooth is not None:
            res["vertices"] = smooth_mesh(res["vertices"], adjacency=adjacency, iterations=n_smooth)
    if normals:
        res["normals"] = mesh_normals(surface, res["vertices"], step=np.asarray(vs, dtype=np.float64).ravel()[:3])
    return res


# ---- evaluating a mesh against another (csrc/gpnerf_meshdist.hip)

def _mesh_tensors(vertices, faces, what):
    for t, name in ((vertices, "vertices"), (faces, "faces")):
        if not isinstance(t, torch.Tensor):
            raise L.GpnerfError(f"{what}: {name} must be a device tensor (mesh_to_device uploads a Mesh)")
        _require_gpu(t, f"{what}: {name}")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_contiguous():
        raise L.GpnerfError(f"{what}: expected contiguous float32 vertices [n,3], got {vertices.dtype} {tuple(vertices.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous() or faces.shape[0] < 1:
        raise L.GpnerfError(f"{what}: expected contiguous int32 faces [m,3], m >= 1, got {faces.dtype} {tuple(faces.shape)}")
    if faces.device != vertices.device:
        raise L.GpnerfError(f"{what}: vertices and faces are on different devices")
    return int(vertices.shape[0]), int(faces.shape[0])


def _points(t, what, like=None):
    _require_gpu(t, what)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
        raise L.GpnerfError(f"{what}: expected a contiguous float32 [n,3] tensor, got {t.dtype} {tuple(t.shape)}")
    if like is not None and t.shape != like.shape:
        raise L.GpnerfError(f"{what}: shape {tuple(t.shape)}, expected {tuple(like.shape)}")
    return t


def mesh_to_device(mesh, device):
    """(vertices float32 [n,3], faces int32 [m,3]) on `device` from a mesh.Mesh, a (vertices, faces) pair of arrays or tensors"""
    v, f = (mesh.vertices, mesh.faces) if hasattr(mesh, "vertices") else mesh
    as_t = lambda a, dt: (a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=device, dtype=dt)
    return as_t(v, torch.float32).reshape(-1, 3).contiguous(), as_t(f, torch.int32).reshape(-1, 3).contiguous()


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
    nv, nf = _mesh_tensors(vertices, faces, "build_mesh_grid")
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
    nv, nf = _mesh_tensors(vertices, faces, "point_mesh_distance")
    points = _points(points, "point_mesh_distance: points")
    if points.device != vertices.device:
        raise L.GpnerfError("point_mesh_distance: points and mesh are on different devices")
    if query_normals is not None:
        query_normals = _points(query_normals, "point_mesh_distance: query_normals", like=points)
    n, dev = int(points.shape[0]), points.device
    res = {"dist": torch.empty((n,), device=dev, dtype=torch.float32), "face": torch.empty((n,), device=dev, dtype=torch.int32)}
    if want_closest:
        res["closest"] = torch.empty((n, 3), device=dev, dtype=torch.float32)
    if query_normals is not None:
        res["cosine"] = torch.empty((n,), device=dev, dtype=torch.float32)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
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
    nv, nf = _mesh_tensors(vertices, faces, "sample_surface")
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
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    L.check(lib.gpnerf_mesh_sample_surface(vertices.data_ptr() or ws.data_ptr(), nv, faces.data_ptr(), nf, n, int(seed) & 0xffffffff, ws.data_ptr(),
                                           ws.numel(), ptr(res["points"]), ptr(res.get("face")), ptr(res.get("normal")), _stream_ptr(dev)),
            "gpnerf_mesh_sample_surface")
    return res


def distance_stats(values, thresholds=(), out=None):
    """gpnerf_distance_stats: one slot (float64 [_lib.DIST_DOUBLES], device) from a device float32 list; out: a slot to write into"""
    lib = L.lib()
    _require_gpu(values, "distance_stats: values")
    if values.dtype != torch.float32 or not values.is_contiguous():
        raise L.GpnerfError(f"distance_stats: expected a contiguous float32 tensor, got {values.dtype}")
    th = [float(t) for t in thresholds]
    if len(th) > L.DIST_MAX_THRESHOLDS:
        raise L.GpnerfError(f"distance_stats: at most {L.DIST_MAX_THRESHOLDS} thresholds")
    if out is None:
        out = torch.empty((L.DIST_DOUBLES,), device=values.device, dtype=torch.float64)
    n = values.numel()
    L.check(lib.gpnerf_distance_stats(values.data_ptr() if n else None, n, (C.c_float * len(th))(*th) if th else None, len(th), out.data_ptr(),
                                      _stream_ptr(values.device)), "gpnerf_distance_stats")
    return out


# ---- registering a mesh onto a scan (csrc/gpnerf_align.hip)

def align_workspace(device):
    """a workspace for rigid_fit / align_mesh's calls (uint8, gpnerf_align_workspace_bytes()); _lib.ALIGN_WS names its doubles"""
    return torch.empty((int(L.lib().gpnerf_align_workspace_bytes()),), device=device, dtype=torch.uint8)


def _slot(out, device, what):
    if out is None:
        return torch.empty((L.XFORM_DOUBLES,), device=device, dtype=torch.float64)
    _require_gpu(out, f"{what}: the slot")
    if out.dtype != torch.float64 or out.numel() != L.XFORM_DOUBLES or not out.is_contiguous() or out.device != device:
        raise L.GpnerfError(f"{what}: the slot is a contiguous float64 [{L.XFORM_DOUBLES}] tensor on {device}, got {out.dtype} "
                            f"{tuple(out.shape)} on {out.device}")
    return out


def rigid_fit(src, dst, weights=None, scale=False, out=None, workspace=None):
    """gpnerf_rigid_fit: the weighted least-squares x -> s R x + t (s = 1 unless scale) that takes the device float32 points src
    [n,3] onto dst [n,3]; weights: device float32 [n] or None.  Returns the transform slot (float64 [_lib.XFORM_DOUBLES] on the
    device; out: a slot to write into); read_transform turns it into a dict.  workspace: an align_workspace to use (its sums stay
    readable behind the call).  Nothing is read back."""
    lib = L.lib()
    src = _points(src, "rigid_fit: src")
    dst = _points(dst, "rigid_fit: dst", like=src)
    n, dev = int(src.shape[0]), src.device
    if dst.device != dev:
        raise L.GpnerfError("rigid_fit: src and dst are on different devices")
    if weights is not None:
        _require_gpu(weights, "rigid_fit: weights")
        if weights.dtype != torch.float32 or weights.shape != (n,) or not weights.is_contiguous() or weights.device != dev:
            raise L.GpnerfError(f"rigid_fit: weights is a contiguous float32 [{n}] tensor on {dev}, got {weights.dtype} {tuple(weights.shape)}")
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
    out = torch.empty_like(points) if out is None else _points(out, "transform_points: out", like=points)
    if out.device != points.device:
        raise L.GpnerfError("transform_points: points and out are on different devices")
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
    nv, nf = _mesh_tensors(vertices, faces, "align_step")
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


# ---- drawing a mesh into calibrated cameras (csrc/gpnerf_raster.hip)

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
    for t, name in ((vertices, "vertices"), (faces, "faces")):
        if not isinstance(t, torch.Tensor):
            raise L.GpnerfError(f"{what}: {name} must be a device tensor (pass a Mesh alone and it is uploaded)")
        _require_gpu(t, f"{what}: {name}")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_contiguous():
        raise L.GpnerfError(f"{what}: expected contiguous float32 vertices [n,3], got {vertices.dtype} {tuple(vertices.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous():
        raise L.GpnerfError(f"{what}: expected contiguous int32 faces [m,3], got {faces.dtype} {tuple(faces.shape)}")
    if faces.device != vertices.device:
        raise L.GpnerfError(f"{what}: vertices and faces are on different devices")
    return vertices, faces


def _raster_cams(Ks, RTs, what):
    host = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    cams = np.ascontiguousarray(np.concatenate([host(Ks).reshape(-1, 9), host(RTs).reshape(-1, 12)], axis=1))
    if not 1 <= cams.shape[0] <= L.RASTER_MAX_VIEWS:
        raise L.GpnerfError(f"{what}: 1 to {L.RASTER_MAX_VIEWS} cameras, got {cams.shape[0]}")
    return cams


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
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    L.check(lib.gpnerf_mesh_rasterize(ptr(vertices), nv, ptr(faces), nf, cams.ctypes.data_as(L.DP), n, H, W, float(z_near), ws.data_ptr(),
                                      ws.numel(), ptr(res.get("depth")), ptr(face_id), res["stats"].data_ptr(), _stream_ptr(dev)),
            "gpnerf_mesh_rasterize")
    if attributes is not None:
        if not isinstance(attributes, torch.Tensor):
            raise L.GpnerfError("rasterize_mesh: attributes must be a device tensor")
        _require_gpu(attributes, "rasterize_mesh: attributes")
        attrs = attributes.reshape(nv, -1) if attributes.dim() == 1 else attributes
        if attrs.dtype != torch.float32 or attrs.dim() != 2 or attrs.shape[0] != nv or not attrs.is_contiguous() or attrs.device != dev:
            raise L.GpnerfError(f"rasterize_mesh: expected contiguous float32 attributes [{nv},C] on {dev}, got {attrs.dtype} {tuple(attrs.shape)}")
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
    for t, name in ((face_id, "face_id"), (masks, "masks")):
        if not isinstance(t, torch.Tensor):
            raise L.GpnerfError(f"silhouette_stats: {name} must be a device tensor")
        _require_gpu(t, f"silhouette_stats: {name}")
    if face_id.dtype != torch.int32 or face_id.dim() != 3 or not face_id.is_contiguous():
        raise L.GpnerfError(f"silhouette_stats: expected contiguous int32 face_id [n,H,W], got {face_id.dtype} {tuple(face_id.shape)}")
    if masks.dtype != torch.uint8 or masks.shape != face_id.shape or not masks.is_contiguous() or masks.device != face_id.device:
        raise L.GpnerfError(f"silhouette_stats: expected contiguous uint8 masks {tuple(face_id.shape)} on {face_id.device}, got {masks.dtype} "
                            f"{tuple(masks.shape)} on {masks.device}")
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
    c = np.asarray(host_counts.detach().cpu() if isinstance(host_counts, torch.Tensor) else host_counts).astype(np.int64).reshape(-1, L.SILHOUETTE_COUNTS)
    if not len(c):
        raise L.GpnerfError("read_silhouette_metrics: no view")
    ratio = lambda num, den: [float(a) / float(b) if b else 1.0 for a, b in zip(c[:, num], c[:, den])]
    per = {"iou": ratio(L.SILHOUETTE_BOTH, L.SILHOUETTE_EITHER), "precision": ratio(L.SILHOUETTE_BOTH, L.SILHOUETTE_COVERED),
           "recall": ratio(L.SILHOUETTE_BOTH, L.SILHOUETTE_GT)}
    res = {k: float(np.mean(v)) for k, v in per.items()}
    per["ignored"] = [int(v) for v in c[:, L.SILHOUETTE_IGNORED]]
    res["per_view"] = per
    return res


# ---- voxelising a mesh: solid occupancy on a lattice, volume and volume IoU (csrc/gpnerf_voxelize.hip)

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
        if not isinstance(points, torch.Tensor):
            raise L.GpnerfError("VoxelGrid.contains: points must be a device tensor")
        pts = _points(points, "VoxelGrid.contains: points")
        if pts.device != self.bits.device:
            raise L.GpnerfError(f"VoxelGrid.contains: points on {pts.device}, the grid on {self.bits.device}")
        n = int(pts.shape[0])
        out = torch.empty((n,), device=self.bits.device, dtype=torch.uint8)
        lat = np.concatenate([self.lo, self.step])
        L.check(L.lib().gpnerf_voxel_contains(self.bits.data_ptr(), self._c_dims(), lat.ctypes.data_as(L.DP), pts.data_ptr() if n else None, n,
                                              out.data_ptr() if n else None, _stream_ptr(self.bits.device)), "gpnerf_voxel_contains")
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
    ptr = lambda t: t.data_ptr() if t.numel() else None
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
    c = np.asarray(host_counts.detach().cpu() if isinstance(host_counts, torch.Tensor) else host_counts).astype(np.int64).reshape(L.VOXEL_COUNTS)
    cell = float(np.prod(np.asarray(step, np.float64).ravel()[:3]))
    ratio = lambda num, den: float(c[num]) / float(c[den]) if c[den] else 1.0
    return {"volume_a": float(c[L.VOXEL_A]) * cell, "volume_b": float(c[L.VOXEL_B]) * cell, "iou": ratio(L.VOXEL_BOTH, L.VOXEL_EITHER),
            "precision": ratio(L.VOXEL_BOTH, L.VOXEL_A), "recall": ratio(L.VOXEL_BOTH, L.VOXEL_B)}


# ---- the truncated signed distance field of a mesh on a lattice (csrc/gpnerf_sdf.hip)

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
        if not isinstance(points, torch.Tensor):
            raise L.GpnerfError("SdfGrid.sample: points must be a device tensor")
        pts = _points(points, "SdfGrid.sample: points")
        _require_gpu(self.values, "SdfGrid.sample: values")
        if pts.device != self.values.device:
            raise L.GpnerfError(f"SdfGrid.sample: points on {pts.device}, the field on {self.values.device}")
        if min(self.dims) < 2:
            raise L.GpnerfError(f"SdfGrid.sample: dims {self.dims} refused (each >= 2)")
        n, dev = int(pts.shape[0]), self.values.device
        out = torch.empty((n,), device=dev, dtype=torch.float32)
        lat = np.concatenate([self.lo, self.step])
        L.check(L.lib().gpnerf_sdf_sample(self.values.data_ptr(), (C.c_int32 * 3)(*self.dims), lat.ctypes.data_as(L.DP),
                                          pts.data_ptr() if n else None, n, out.data_ptr() if n else None, _stream_ptr(dev)), "gpnerf_sdf_sample")
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
    ptr = lambda t: t.data_ptr() if t.numel() else None
    L.check(lib.gpnerf_mesh_sdf(ptr(vertices), nv, ptr(faces), nf, lat.ctypes.data_as(L.DP), cd, band32,
                                voxels.bits.data_ptr() if voxels is not None else None, ws.data_ptr(), ws.numel(), values.data_ptr(),
                                face.data_ptr() if face is not None else None, stats.data_ptr(), _stream_ptr(dev)), "gpnerf_mesh_sdf")
    return SdfGrid(values, face, voxels, lat[:3], lat[3:], d, band32, stats)


# ---- casting rays against a mesh (csrc/gpnerf_raycast.hip)

def _rays(t, what):
    if not isinstance(t, torch.Tensor):
        raise L.GpnerfError(f"{what} must be a device tensor")
    _require_gpu(t, what)
    if t.dtype != torch.float32 or t.dim() < 1 or t.shape[-1] != 8 or not t.is_contiguous():
        raise L.GpnerfError(f"{what}: expected a contiguous float32 [...,8] tensor of (o, d, tmin, tmax) rows, got {t.dtype} {tuple(t.shape)}")
    return t


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
    nv, nf = _mesh_tensors(vertices, faces, "raycast_mesh")
    rays = _rays(rays, "raycast_mesh: rays")
    if rays.device != vertices.device:
        raise L.GpnerfError("raycast_mesh: rays and mesh are on different devices")
    shape, dev = tuple(rays.shape[:-1]), rays.device
    n = int(np.prod(shape, dtype=np.int64))
    res = {"t": torch.empty(shape, device=dev, dtype=torch.float32), "face": torch.empty(shape, device=dev, dtype=torch.int32)}
    if want_bary:
        res["bary"] = torch.empty(shape + (2,), device=dev, dtype=torch.float32)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
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


# ---- colouring points from calibrated views (csrc/gpnerf_texture.hip)

TEXTURE_WANT = ("color", "weight", "views")


def face_vertex_normals(vertices, faces):
    """Area-weighted vertex normals of a device mesh -> float32 [n,3], not normalised: every face's cross product (b - a) x (c - a) in
    float64, added to its three vertices by index_add_ in face order.  A vertex no face names gets the zero vector."""
    nv, _ = _mesh_tensors(vertices, faces, "face_vertex_normals")
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
    if not isinstance(points, torch.Tensor) or not isinstance(images, torch.Tensor):
        raise L.GpnerfError("texture_points: points and images must be device tensors")
    points = _points(points, "texture_points: points")
    dev, n = points.device, int(points.shape[0])
    cams = _raster_cams(Ks, RTs, "texture_points")
    m = cams.shape[0]
    _require_gpu(images, "texture_points: images")
    if images.dtype != torch.float32 or images.dim() != 4 or images.shape[0] != m or not images.is_contiguous() or images.device != dev:
        raise L.GpnerfError(f"texture_points: expected contiguous float32 images [{m},H,W,C] on {dev}, got {images.dtype} {tuple(images.shape)}")
    H, W, c = (int(s) for s in images.shape[1:])
    if not 1 <= c <= L.TEXTURE_MAX_CHANNELS:
        raise L.GpnerfError(f"texture_points: 1 to {L.TEXTURE_MAX_CHANNELS} channels, got {c}")
    if normals is not None:
        normals = _points(normals, "texture_points: normals", like=points)
    if masks is not None:
        if not isinstance(masks, torch.Tensor) or not masks.is_cuda or masks.dtype != torch.uint8 or tuple(masks.shape) != (m, H, W) \
                or not masks.is_contiguous():
            raise L.GpnerfError(f"texture_points: expected contiguous uint8 masks [{m},{H},{W}] on the GPU")
    if fallback is not None:
        if not isinstance(fallback, torch.Tensor) or not fallback.is_cuda or fallback.dtype != torch.float32 \
                or tuple(fallback.shape) != (n, c) or not fallback.is_contiguous():
            raise L.GpnerfError(f"texture_points: expected a contiguous float32 fallback [{n},{c}] on the GPU")
    for t, name in ((normals, "normals"), (masks, "masks"), (fallback, "fallback")):
        if t is not None and t.device != dev:
            raise L.GpnerfError(f"texture_points: points and {name} are on different devices")
    nv = nf = 0
    if grid is not None:
        if not isinstance(grid, MeshGrid):
            raise L.GpnerfError("texture_points: grid must be a MeshGrid (build_mesh_grid)")
        vertices, faces = grid.vertices, grid.faces
    if vertices is not None or faces is not None:
        nv, nf = _mesh_tensors(vertices, faces, "texture_points")
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
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
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
    _mesh_tensors(vertices, faces, "texture_mesh")
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
    host = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a).astype(np.int64)
    s, t = host(stats).reshape(-1, L.TEXTURE_FATES), host(totals).reshape(2)
    n = int(t.sum())
    res = {"per_view": {name: [int(v) for v in s[:, k]] for k, name in enumerate(L.TEXTURE_STATS)}}
    res["used_fraction"] = [float(u) / n if n else 0.0 for u in s[:, L.TEXTURE_USED]]
    res["seen"], res["unseen"] = int(t[0]), int(t[1])
    res["seen_fraction"] = float(t[0]) / n if n else 0.0
    return res


# ---- a per-face texture atlas (csrc/gpnerf_atlas.hip)

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
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != nv or not t.is_contiguous() \
            or t.device != dev or (channels is not None and t.shape[1] != channels):
        raise L.GpnerfError(f"{what}: expected a contiguous float32 [{nv},{channels or 'C'}] tensor on {dev}")
    return t


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
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
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
        if not isinstance(face_id, torch.Tensor) or not face_id.is_cuda or face_id.dtype != torch.int32 or face_id.dim() != 3 \
                or face_id.shape[0] != n or not face_id.is_contiguous() or face_id.device != dev:
            raise L.GpnerfError(f"TextureAtlas.shade: expected a contiguous int32 face_id [{n},H,W] on {dev}")
        H, W = int(face_id.shape[1]), int(face_id.shape[2])
        c = int(self.image.shape[2])
        bg = np.broadcast_to(np.asarray(background, dtype=np.float32), (c,))
        out = torch.empty((n, H, W, c), device=dev, dtype=torch.float32)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
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
    if not isinstance(colors, torch.Tensor) or not colors.is_cuda or colors.dtype != torch.float32 or colors.dim() != 2 or colors.shape[0] != t \
            or not colors.is_contiguous() or not 1 <= colors.shape[1] <= L.TEXTURE_MAX_CHANNELS:
        raise L.GpnerfError(f"atlas_pack: expected contiguous float32 colors [{t},C] on the GPU, C <= {L.TEXTURE_MAX_CHANNELS}")
    dev, c = colors.device, int(colors.shape[1])
    if views is not None and (not isinstance(views, torch.Tensor) or views.dtype != torch.uint8 or tuple(views.shape) != (t,)
                              or not views.is_contiguous() or views.device != dev):
        raise L.GpnerfError(f"atlas_pack: expected contiguous uint8 views [{t}] on {dev}")
    bg = np.broadcast_to(np.asarray(background, dtype=np.float32), (c,))
    image = torch.empty((lay["height"], lay["width"], c), device=dev, dtype=torch.float32)
    coverage = torch.empty((lay["height"], lay["width"]), device=dev, dtype=torch.uint8)
    ptr = lambda a: a.data_ptr() if a is not None and a.numel() else None
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
    nv, nf = _mesh_tensors(vertices, faces, "texture_atlas")
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
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise L.GpnerfError("texture_atlas: images must be a device tensor [m,H,W,C]")
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


# ---- fusing depth maps into a truncated signed distance field (csrc/gpnerf_fusion.hip)

def _fusion_band(band, lat, what):
    band32 = float(np.float32(band))
    if not (np.isfinite(band32) and 0.0 < band32 <= L.SDF_MAX_BAND_STEPS * float(lat[3:].min())):
        raise L.GpnerfError(f"{what}: band {band} refused (finite, > 0, at most {L.SDF_MAX_BAND_STEPS} x the smallest step {float(lat[3:].min())})")
    return band32


def _fusion_views(depth, Ks, RTs, weights, z_near, what, dev=None):
    """the checked (depth, weights, cams, n_views, H, W, z_near) of a fusion call"""
    if not isinstance(depth, torch.Tensor):
        raise L.GpnerfError(f"{what}: depth must be a device tensor")
    _require_gpu(depth, f"{what}: depth")
    cams = _raster_cams(Ks, RTs, what)
    m = cams.shape[0]
    if depth.dtype != torch.float32 or depth.dim() != 3 or depth.shape[0] != m or not depth.is_contiguous() or 0 in depth.shape:
        raise L.GpnerfError(f"{what}: expected contiguous float32 depth [{m},H,W], got {depth.dtype} {tuple(depth.shape)}")
    if dev is not None and depth.device != dev:
        raise L.GpnerfError(f"{what}: depth on {depth.device}, the lattice's state on {dev}")
    H, W = int(depth.shape[1]), int(depth.shape[2])
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise L.GpnerfError(f"{what}: refused ({m} views, {H} x {W})")
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or not weights.is_cuda or weights.dtype != torch.float32 \
                or tuple(weights.shape) != (m, H, W) or not weights.is_contiguous() or weights.device != depth.device:
            got = f"{weights.dtype} {tuple(weights.shape)}" if isinstance(weights, torch.Tensor) else type(weights).__name__
            raise L.GpnerfError(f"{what}: expected contiguous float32 weights [{m},{H},{W}] on {depth.device}, got {got}")
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
    host = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a).astype(np.int64)
    s, t = host(stats).reshape(-1, L.FUSION_N_FATES), host(totals).reshape(L.FUSION_N_TOTALS)
    res = {"per_view": {name: [int(v) for v in s[:, k]] for k, name in enumerate(L.FUSION_FATES)}}
    res.update({name: int(t[k]) for k, name in enumerate(L.FUSION_TOTALS)})
    n = int(t[L.FUSION_SEEN] + t[L.FUSION_INTERIOR] + t[L.FUSION_UNKNOWN])
    res["seen_fraction"] = float(t[L.FUSION_SEEN]) / n if n else 0.0
    return res
