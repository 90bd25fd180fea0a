"""`Evaluator` with the reference's interface (libs/evaluators/if_nerf.py:8-88), computing on the tensors' device
(SURVEY.md §8f-4): `evaluate(output, batch)` accumulates MSE / PSNR / SSIM of one rendered view, `summarize()` returns
and prints their means and resets.

PSNR = -10 log10(mean((pred - gt)^2)) over the `mask_at_box` pixels (if_nerf.py:15-18,59-63).
SSIM follows the call the reference makes, `skimage.measure.compare_ssim(pred, gt, multichannel=True)` on the
bounding-box crop of the mask with both images zero outside it (if_nerf.py:20-47): 7x7 uniform window, sample
covariance (x 49/48), K1 = 0.01, K2 = 0.03, data range 2 (skimage's range for float images), mean over the map cropped by
3 pixels and over channels.  scikit-image is not installed in this image, so that part is a restatement of the published
algorithm: **parity unpinned** (tests check it against a scipy `uniform_filter` restatement).
Image writing (cfg.test.save_imgs) is I/O and out of scope.

`evaluate_loop` is the evaluation loop around it (libs/trainers/BaseTrainer.py:255-280 `Trainer.evaluate`): per frame
`render.render(batch)` -> `Evaluator.evaluate`, the render time summed from `ret["rtime"]`, the means from `summarize()`;
pinned to the reference's own loop over three frames (tests/golden/loop_demo_3frames.npz).

`MeshEvaluator` mirrors libs/evaluators/if_nerf_mesh.py for a geometry-mode renderer (use_rgbhead False); the loop takes it
through `evaluate_loop(evaluator=...)` and otherwise constructs the image evaluator, as the reference's loop always does.  Given a
`gt_mesh` per frame it also computes the geometry metrics (P2S, Chamfer, normal consistency, F-score) on the device
(frame.mesh_metrics, csrc/gpnerf_meshdist.hip); with `silhouette=True` and the cameras and masks of the dense renderer's geometry mode
in the batch it scores the mesh's silhouettes against the masks (frame.rasterize_mesh, csrc/gpnerf_raster.hip): what data without
scans offers.

`DeviceEvaluator` (opt-in: `evaluate_loop(device_metrics=True)` or GPNERF_DEVICE_METRICS=1) computes the same three numbers with
gpnerf_image_metrics (csrc/gpnerf_metrics.hip): four kernel launches per frame into a device slot, no host synchronisation in
`evaluate`; the host reads every frame's slot in one copy when `.mse` / `.psnr` / `.ssim` are first asked for.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L

_WIN, _K1, _K2, _RANGE = 7, 0.01, 0.03, 2.0


def psnr_metric(pred, gt):
    """pred, gt: tensors of equal shape -> python float (if_nerf.py:15-18)."""
    mse = torch.mean((pred.double() - gt.double()) ** 2).item()
    return -10.0 * math.log(mse) / math.log(10.0) if mse > 0 else float("inf")


def ssim_images(a, b):
    """Mean SSIM of two [H,W,C] images (skimage compare_ssim defaults, multichannel).  float64 on the inputs' device."""
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"expected two [H,W,C] images, got {tuple(a.shape)} and {tuple(b.shape)}")
    if min(a.shape[0], a.shape[1]) < _WIN:
        raise ValueError("win_size exceeds image extent")      # skimage raises the same
    x = a.double().permute(2, 0, 1).unsqueeze(1)              # [C,1,H,W]
    y = b.double().permute(2, 0, 1).unsqueeze(1)
    box = lambda t: F.avg_pool2d(t, _WIN, stride=1)           # valid window means == the map cropped by (win-1)/2
    ux, uy = box(x), box(y)
    norm = _WIN * _WIN / (_WIN * _WIN - 1.0)
    vx, vy, vxy = norm * (box(x * x) - ux * ux), norm * (box(y * y) - uy * uy), norm * (box(x * y) - ux * uy)
    c1, c2 = (_K1 * _RANGE) ** 2, (_K2 * _RANGE) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s.mean(dim=(1, 2, 3)).mean().item()


def mask_bounding_rect(mask):
    """(x, y, w, h) of the non-zero pixels of a [H,W] bool tensor (what cv2.boundingRect returns); (0,0,0,0) if empty."""
    rows = torch.nonzero(mask.any(dim=1)).flatten()
    cols = torch.nonzero(mask.any(dim=0)).flatten()
    if rows.numel() == 0:
        return 0, 0, 0, 0
    y0, y1, x0, x1 = int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


class Evaluator:
    def __init__(self, cfg, seq_name):
        self.cfg, self.seq_name = cfg, seq_name
        self.mse, self.psnr, self.ssim = [], [], []

    def _hw(self):
        d = self.cfg.dataset
        return int(d.H * d.ratio), int(d.W * d.ratio)

    def psnr_metric(self, img_pred, img_gt):
        return psnr_metric(torch.as_tensor(img_pred), torch.as_tensor(img_gt))

    def ssim_metric(self, rgb_pred, rgb_gt, batch):
        H, W = self._hw()
        rgb_pred, rgb_gt = torch.as_tensor(rgb_pred), torch.as_tensor(rgb_gt)
        mask = torch.as_tensor(batch["mask_at_box"][0]).reshape(H, W).to(rgb_pred.device).bool()
        pred = torch.zeros((H, W, 3), dtype=torch.float64, device=rgb_pred.device)
        gt = torch.zeros_like(pred)
        pred[mask] = rgb_pred.double()
        gt[mask] = rgb_gt.to(rgb_pred.device).double()
        x, y, w, h = mask_bounding_rect(mask)
        return ssim_images(pred[y:y + h, x:x + w], gt[y:y + h, x:x + w])

    def evaluate(self, output, batch):
        if "pred_img" not in output:
            rgb_pred = torch.as_tensor(output["rgb_map"][0]).detach()
        else:                                                     # progressive renderer (demo_render.py:359-364)
            H, W = self._hw()
            mask = torch.as_tensor(batch["mask_at_box"][0]).reshape(H, W).bool()
            img = torch.as_tensor(output["pred_img"])
            rgb_pred = img[mask.to(img.device)]
        rgb_gt = torch.as_tensor(batch["rgb"][0]).detach().to(rgb_pred.device)
        self.mse.append(torch.mean((rgb_pred.double() - rgb_gt.double()) ** 2).item())
        self.psnr.append(psnr_metric(rgb_pred, rgb_gt))
        self.ssim.append(self.ssim_metric(rgb_pred, rgb_gt, batch))

    def summarize(self):
        metrics = {"mse": float(np.mean(self.mse)), "psnr": float(np.mean(self.psnr)), "ssim": float(np.mean(self.ssim))}
        result_dir = getattr(self.cfg, "result_dir", None)
        if result_dir:                                            # if_nerf.py:72-80 keeps the per-view MSE list
            path = os.path.join(result_dir, self.seq_name, "metrics.npy")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.save(path, self.mse)
        for k in ("mse", "psnr", "ssim"):
            print(f"{k}: {metrics[k]}")
        self.mse, self.psnr, self.ssim = [], [], []
        return metrics


class DeviceEvaluator(Evaluator):
    """`Evaluator` whose `evaluate` only enqueues: gpnerf_image_metrics on `torch.cuda.current_stream()` writes the frame's MSE, SSIM,
    bounding rectangle, population and status into slot k of a results buffer (chunks of `CHUNK` slots; a full buffer grows by one
    more chunk, nothing is copied), with one workspace per (stream, H, W): no allocation per frame after the first, no synchronisation.
    `.mse`, `.psnr`, `.ssim` are read lazily: the first read after an `evaluate` waits for the stream(s), copies the filled slots
    to the host once and turns them into the Python lists `Evaluator` keeps (PSNR by `psnr_metric`'s formula from the slot's MSE).
    A frame whose status is not 0 raises at that read what the torch path raises at `evaluate` -- ValueError("win_size exceeds
    image extent") for an empty mask or a bounding rectangle under 7 pixels, a ValueError naming the two counts where the mask's
    population is not the number of pixels handed in -- once; the frame is dropped and the other frames keep their numbers.
    Inputs are float32 CUDA tensors (CPU tensors are refused: there is no fallback); an output with `pred_img` (the progressive
    renderer's host arrays) goes through the inherited torch path, in frame order.
    Input lifetime: the kernels read `rgb_map`, `rgb` and the mask in stream order.  Renderer.render's outputs come from torch's
    caching allocator, which hands a freed block to a later allocation of the SAME stream only -- behind the kernels when that is the
    stream `evaluate` ran on; a tensor that belongs to another stream is held back by record_stream (a no-op on the tensor's own)."""
    CHUNK = 1024

    def __init__(self, cfg, seq_name):
        self._lists = {"mse": [], "psnr": [], "ssim": []}
        self._pending = []                # (index in the lists, chunk, slot, n) of the frames whose slots have not been read
        self._chunks, self._filled = [], 0
        self._workspaces, self._streams = {}, {}
        super().__init__(cfg, seq_name)

    def _get(name):
        def get(self):
            self._drain()
            return self._lists[name]

        def put(self, value):
            self._lists[name] = value
        return property(get, put)

    mse, psnr, ssim = _get("mse"), _get("psnr"), _get("ssim")
    del _get

    def evaluate(self, output, batch):
        if "pred_img" in output:
            return super().evaluate(output, batch)                # (reads the lists: pending slots are drained first, the order holds)
        rgb_pred = torch.as_tensor(output["rgb_map"][0]).detach()
        rgb_gt = torch.as_tensor(batch["rgb"][0]).detach()
        mask = torch.as_tensor(batch["mask_at_box"][0])
        for name, t in (("rgb_map", rgb_pred), ("rgb", rgb_gt), ("mask_at_box", mask)):
            if not t.is_cuda:
                raise ValueError(f"DeviceEvaluator: {name} is a CPU tensor (no CPU fallback: use Evaluator)")
        dev = rgb_pred.device
        if rgb_gt.device != dev or mask.device != dev:
            raise ValueError("DeviceEvaluator: rgb_map, rgb and mask_at_box are on different devices")
        if rgb_pred.dtype != torch.float32 or rgb_gt.dtype != torch.float32:
            raise ValueError(f"DeviceEvaluator: float32 colours expected, got {rgb_pred.dtype} and {rgb_gt.dtype}")
        if rgb_pred.dim() != 2 or rgb_pred.shape[1] != 3 or rgb_gt.shape != rgb_pred.shape:
            raise ValueError(f"expected two [n,3] colour lists, got {tuple(rgb_pred.shape)} and {tuple(rgb_gt.shape)}")
        H, W = self._hw()
        mask = mask.reshape(H * W)
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask if mask.dtype == torch.uint8 else (mask != 0).view(torch.uint8)
        rgb_pred, rgb_gt, mask = rgb_pred.contiguous(), rgb_gt.contiguous(), mask.contiguous()
        n = int(rgb_pred.shape[0])
        lib = L.lib()
        stream = torch.cuda.current_stream(dev)
        key = (stream.cuda_stream, H, W)                          # (a workspace serves one stream's calls, which run in order)
        ws = self._workspaces.get(key)
        if ws is None:
            ws = self._workspaces[key] = torch.empty((int(lib.gpnerf_metrics_workspace_bytes(H, W)),), device=dev, dtype=torch.uint8)
        chunk, slot = divmod(self._filled, self.CHUNK)
        if chunk == len(self._chunks):
            self._chunks.append(torch.empty((self.CHUNK, L.METRICS_DOUBLES), device=dev, dtype=torch.float64))
        elif self._chunks[chunk].device != dev:
            raise ValueError("DeviceEvaluator: one evaluator serves one device")
        for t in (rgb_pred, rgb_gt, mask):
            t.record_stream(stream)
        out = self._chunks[chunk].data_ptr() + slot * L.METRICS_DOUBLES * 8
        # (an empty tensor has no address; the entry point refuses null pointers, and with n = 0 it reads neither list)
        L.check(lib.gpnerf_image_metrics(rgb_pred.data_ptr() or ws.data_ptr(), rgb_gt.data_ptr() or ws.data_ptr(), mask.data_ptr(), H, W, n,
                                         ws.data_ptr(), ws.numel(), out, stream.cuda_stream), "gpnerf_image_metrics")
        self._streams[stream.cuda_stream] = stream
        self._pending.append((len(self._lists["mse"]), chunk, slot, n))
        self._filled += 1
        for v in self._lists.values():
            v.append(None)

    def _drain(self):
        if not self._pending:
            return
        for s in self._streams.values():
            s.synchronize()
        full, rest = divmod(self._filled, self.CHUNK)
        host = [c[:self.CHUNK if i < full else rest].cpu().numpy() for i, c in enumerate(self._chunks[:full + (1 if rest else 0)])]
        pending, self._pending, self._filled, self._streams = self._pending, [], 0, {}
        bad = []
        for at, chunk, slot, n in pending:
            r = host[chunk][slot]
            status = int(r[L.METRICS_STATUS])
            if status:
                bad.append((at, status, int(r[L.METRICS_POPULATION]), n))
                continue
            mse = float(r[L.METRICS_MSE])
            self._lists["mse"][at] = mse
            self._lists["psnr"][at] = -10.0 * math.log(mse) / math.log(10.0) if mse > 0 else float("inf")
            self._lists["ssim"][at] = float(r[L.METRICS_SSIM])
        if bad:
            for at, _, _, _ in reversed(bad):
                for v in self._lists.values():
                    del v[at]
            at, status, pop, n = bad[0]
            if status == 1:
                raise ValueError(f"frame {at}: mask_at_box has {pop} pixels set, rgb_map has {n}")
            raise ValueError("win_size exceeds image extent")


class MeshEvaluator:
    """The geometry mode's evaluator (libs/evaluators/if_nerf_mesh.py): `evaluate` saves the lattice points whose alpha is above
    `mesh_th` to `<result_path>/pts/<frame_index>.npy`, `visualize` exports the mesh to `<result_path>/mesh/<frame_index>.ply`
    (`..._cam<c>.ply` when the batch has `cam_ind`).  `output` is what Renderer.render returns with use_rgbhead False.  The
    directories are made with os.makedirs (the reference shells out to mkdir -p and announces them through termcolor).
    export_mesh (not in the reference, whose loop never calls visualize): `evaluate` also calls `visualize`, so that an evaluation
    loop leaves the meshes behind.
    Metrics (not in the reference, which has `# TODO evaluate mesh` at if_nerf_mesh.py:32): a batch with `gt_mesh` -- a mesh.Mesh or
    a (vertices, faces) pair in the frame of the lattice axes -- makes `evaluate` enqueue frame.mesh_metrics of the frame's mesh
    against it (no host read; the predicted mesh goes through `to_lattice_frame(output["axes"], PAD)` when the output has `axes`
    and is taken as it is otherwise) and keep the slots.  `summarize()` reads all slots in one copy and returns the per-key means
    over the frames, with the per-frame lists under "per_frame", saves those lists as `<result_path>/mesh_metrics.npy` (next to
    pts/) and resets.  With no `gt_mesh` ever seen it returns {} and writes nothing, as the reference does.
    metric_samples: surface samples per mesh and direction; metric_thresholds: the F-score distances, in the meshes' unit (metres
    for the project's scenes: 5 mm, 1 cm, 2 cm); metric_max_dist: gpnerf_mesh_distance's max_dist (inf: exact everywhere);
    metric_cell_cap, metric_entry_cap: the grids' capacities (None: frame.mesh_grid_caps).  `evaluate` does not read the grids'
    status, so a grid that overflows its entry capacity shows at `summarize()`, whose error says how to find the capacity to pass here.
    align (None by default; "rigid"): the frame's mesh is first registered onto `gt_mesh` on the device (frame.align_mesh through
    frame.mesh_metrics(align="rigid"): `align_iterations` trimmed point-to-plane steps, pairs beyond `align_max_dist` trimmed; still
    no host read per frame), so the geometry metrics are those AFTER registration -- a scan sits millimetres to centimetres off the
    lattice frame, which at 5 mm decides the F-score.  `summarize()` then adds per frame `align_rms`, `align_rotation_deg`,
    `align_translation` (the length of the translation) and `align_status` (0 ok, 1 few, 2 singular), their means but for the
    status, and saves the 4 x 4 matrices as `<result_path>/align_transforms.npy` [frames, 4, 4].  With None the keys and files are
    what they are without the keyword.
    silhouette (off by default; data with cameras and masks but no scan): a batch with `hull_masks` [1,n,h,w] uint8 (0, 1, border
    100), `hull_Ks` [1,n,3,3] and `hull_RTs` [1,n,3,4] -- the keys of the dense renderer's geometry mode -- makes `evaluate` put the
    frame's mesh through `to_lattice_frame(output["axes"], PAD)`, draw it into those cameras at the masks' size
    (frame.rasterize_mesh) and enqueue frame.silhouette_stats against the masks: a slot per frame, no host read.  `summarize()`
    reads the slots in one copy and adds `silhouette_iou`, `silhouette_precision`, `silhouette_recall` (means over views and
    frames; the border band is left out) and their per-frame lists, and saves `<result_path>/silhouette_metrics.npy` (a structured
    array: frame_index, the three means, and the per-view values).  An output without `axes` -- the inference renderer's
    render_mesh, whose mesh is not in the cameras' frame -- raises a GpnerfError naming the key.  Off, nothing changes.
    topology (off by default; needs neither scan nor masks): `evaluate` uploads the frame's mesh and enqueues frame.mesh_topology, a
    slot of ten counts (_lib.TOPOLOGY_STATS) per frame, no host read.  `summarize()` reads the slots in one copy and adds
    `watertight_frames` (how many frames' meshes are closed and oriented), `topology_<name>` for the edge counts and `euler` (means
    over the frames) and their per-frame lists, and saves `<result_path>/topology_metrics.npy` (a structured array: frame_index, the
    ten counts, closed, oriented, watertight).
    components (off by default; a knob of its own, so that topology=True's keys and file stay what they are): `evaluate` uploads the
    frame's mesh and enqueues frame.mesh_components (every component kept), a slot per frame of the nine counts
    (_lib.COMPONENT_STATS), the largest component's boundary vertices and the mesh's non-manifold and inconsistent edges; no host
    read per frame.  `summarize()` reads the slots in one copy and adds `components_mean` (pieces per frame), `single_component_frames`
    and the per-frame lists `components`, `components_largest_faces`, `components_largest_genus` and `components_frame_index`, and
    saves `<result_path>/components_metrics.npy` (a structured array: frame_index, the nine counts, and largest_genus, the genus of
    the largest component by frame.read_mesh_components' rule, -1 where it is not defined).  It is the first thing to look at when a
    sequence's Chamfer distance or volume IoU jumps on one frame.
    volume (off by default; the third standard reconstruction number beside Chamfer and normal consistency, and the one that compares
    solids): a batch with `gt_mesh` and an output with `axes` make `evaluate` voxelise both meshes on the frame's padded cube lattice
    (frame.voxelize_mesh, rule `volume_rule`: "nonzero" unites a scan's separate parts, "parity" is indifferent to orientation) -- the
    predicted mesh as it is exported, in index units (lo 0, step 1), the scan with lo = axes[a][0] - PAD * step_a and the axes' steps,
    to_lattice_frame's -- and enqueue frame.voxel_stats into a slot: no host read.  `summarize()` reads the slots in one copy and adds
    `volume_iou`, `volume_pred`, `volume_gt` (the volumes in the axes' unit cubed; means over the frames) and
    `volume_open_columns_pred` / `_gt` (lattice columns through which a mesh leaks: more than 0 says it is not closed, and its volume
    is not to be trusted there), their per-frame lists, and saves `<result_path>/volume_metrics.npy`.  A `gt_mesh` with an output
    that has no `axes` raises a GpnerfError naming the key.  Off, nothing changes.
    signed (off by default; P2S and Chamfer say how far the reconstruction is from the scan, never on which side: "bloated" and
    "shrunk" score the same): like `volume` it needs `gt_mesh` in the batch and `axes` in the output.  `evaluate` builds the scan's
    truncated signed distance field on the frame's padded cube lattice (frame.mesh_sdf, rule `volume_rule`, a band of `signed_band`
    lattice steps -- times the smallest step), draws `metric_samples` surface samples of the predicted mesh in that frame
    (to_lattice_frame, frame.sample_surface), samples the field there (SdfGrid.sample) and reduces the values with
    frame.distance_stats at threshold 0 into a slot: no host read.  `summarize()` reads the slots in one copy and adds
    `signed_mean` (positive: the prediction lies outside the scan), `inside_fraction` (the share of the samples with a value <= 0)
    and `signed_outside_lattice` (samples outside the padded lattice, which take no part), their per-frame lists, and saves
    `<result_path>/signed_metrics.npy`.  Values beyond the band saturate at +-band, so `signed_mean` is a truncated mean: it is the
    true signed mean while the surfaces are within the band of each other, and an under-estimate in size (never in sign) beyond.
    Off, nothing changes.
    visible (off by default; the visible-surface error depth evaluations report -- P2S and Chamfer average over hidden surface too):
    it needs `gt_mesh` in the batch, `axes` in the output and the `hull_masks` / `hull_Ks` / `hull_RTs` keys `silhouette` uses (only
    the masks' size is read).  `evaluate` casts the hull cameras' pixel rays (frame.pixel_rays at the masks' size) against the
    predicted mesh (`to_lattice_frame`) and against the scan, each through its own grid (frame.raycast_mesh), forms |t_pred - t_gt|
    on the device -- NaN where neither is hit, +inf where exactly one is -- and reduces it with frame.distance_stats into a slot: no
    host read.  `summarize()` reads the slots in one copy and adds `visible_depth_mean`, `visible_depth_rms`, `visible_depth_max`
    (camera depth, the meshes' unit, over the pixels where both are hit; means over the frames, the max over them),
    `visible_hit_disagreement` (the share of the pixels hit by exactly one mesh among those hit by either), their per-frame lists,
    and saves `<result_path>/visible_metrics.npy`.  A `gt_mesh` with an output that has no `axes`, or a batch without one of the
    three keys, raises a GpnerfError naming the key.  Off, nothing changes.
    texture (off by default; the photometric score of a mesh, the colour counterpart of the silhouette IoU): it needs `axes` in the
    output, the `hull_masks` / `hull_Ks` / `hull_RTs` keys and `hull_imgs` [1,n,h,w,3] float32 in [0,1], the cameras' images.
    `evaluate` puts the frame's mesh into the cameras' frame (`to_lattice_frame`), colours its vertices from the hull views whose
    index is not a multiple of `texture_holdout` (the first 8 of them; frame.texture_mesh, masked, hidden by the mesh itself), draws
    the coloured mesh into the held-out views (frame.rasterize_mesh with the colours as attributes; the first 8), forms the
    difference to their images on the device -- NaN where no face covers the pixel or the mask is not 1 -- and reduces it with
    frame.distance_stats into a slot: no host read (the mesh's grid is built unchecked).  `summarize()` reads the slots in one copy
    and adds `texture_psnr` (-10 log10 of the mean square over the counted pixels' channels; the mean over the frames),
    `texture_pixels` (counted pixels, summed), `texture_seen_fraction` (the share of the vertices some colouring view saw), their
    per-frame lists, and saves `<result_path>/texture_metrics.npy`.  A missing key raises a GpnerfError naming it.  Off, nothing
    changes.  texture="atlas" runs the same protocol -- the same views, slots, keys and table -- with a per-face texture atlas of
    `texture_res` texels per face edge in place of the vertex colours: frame.texture_atlas bakes it from the colouring views (the
    faces' own normals), TextureAtlas.shade draws the held-out views, and `texture_seen_fraction` is the seen share of the owned
    texels (the table's vertices_seen / vertices_unseen then count texels).
    repair_gt (off by default; repair_tol, 0.0 by default, is its weld tolerance): a batch's `gt_mesh` goes through frame.repair_mesh
    once per frame -- welded, repeated and unusable faces dropped, every patch wound outward -- before any metric above sees it: a
    scanner's triangle soup or a merged export otherwise makes the signed metrics, the volume IoU and the normal consistency wrong
    without saying so.  One host read per frame (the repaired mesh's two sizes).  `summarize()` adds `gt_repaired_frames` (frames whose
    scan the repair changed), the per-frame lists `gt_repair_<name>` (_lib.REPAIR_STATS and `changed`) and `gt_repair_frame_index`,
    and saves `<result_path>/repair_metrics.npy` (a structured array: frame_index, the sixteen counts, changed).  Off, no launch is
    added, no key appears and every output is what it is without the keyword."""
    PAD = 10                              # if_nerf_mesh.py:20, the np.pad(cube, 10) of BaseRender.py:269

    def __init__(self, result_path, mesh_th, export_mesh=False, metric_samples=100000, metric_thresholds=(0.005, 0.01, 0.02),
                 metric_max_dist=float("inf"), metric_device=None, metric_cell_cap=None, metric_entry_cap=None, silhouette=False,
                 topology=False, volume=False, volume_rule="nonzero", components=False, align=None, align_iterations=10,
                 align_max_dist=float("inf"), signed=False, signed_band=8, visible=False, texture=False, texture_holdout=4,
                 texture_res=8, repair_gt=False, repair_tol=0.0):
        self.mesh_th = mesh_th
        self.repair_gt, self.repair_tol = bool(repair_gt), float(repair_tol)
        if not 0.0 <= self.repair_tol < float("inf"):
            raise L.GpnerfError(f"MeshEvaluator: repair_tol must be finite and >= 0, got {repair_tol!r}")
        self._repair_slots, self._repair_frames = [], []
        self.export_mesh = bool(export_mesh)
        self.result_path = result_path
        self.vis_result_dir = os.path.join(result_path, "mesh")
        self.pts_result_dir = os.path.join(result_path, "pts")
        self.metric_samples, self.metric_thresholds = int(metric_samples), tuple(float(t) for t in metric_thresholds)
        self.metric_max_dist, self.metric_device = float(metric_max_dist), metric_device
        self.metric_cell_cap, self.metric_entry_cap = metric_cell_cap, metric_entry_cap
        self._slots, self._frames = [], []
        if align not in (None, "rigid"):
            raise L.GpnerfError(f"MeshEvaluator: align is None or 'rigid', got {align!r}")
        self.align, self.align_iterations, self.align_max_dist = align, int(align_iterations), float(align_max_dist)
        self._transforms = []
        self.silhouette = bool(silhouette)
        self._sil_slots, self._sil_frames = [], []
        self.topology = bool(topology)
        self._topo_slots, self._topo_frames = [], []
        self.components = bool(components)
        self._comp_slots, self._comp_frames = [], []
        self.volume, self.volume_rule = bool(volume), str(volume_rule)
        if self.volume_rule not in L.VOXEL_RULES:
            raise L.GpnerfError(f"MeshEvaluator: volume_rule is 'parity' or 'nonzero', got {volume_rule!r}")
        self._vol_slots, self._vol_frames, self._vol_cells = [], [], []
        self.signed, self.signed_band = bool(signed), float(signed_band)
        if not 0.0 < self.signed_band <= L.SDF_MAX_BAND_STEPS:
            raise L.GpnerfError(f"MeshEvaluator: signed_band is in lattice steps, > 0 and at most {L.SDF_MAX_BAND_STEPS}, got {signed_band!r}")
        self._signed_slots, self._signed_frames = [], []
        self.visible = bool(visible)
        self._visible_slots, self._visible_frames = [], []
        if texture not in (False, True, None, 0, 1, "atlas"):
            raise L.GpnerfError(f"MeshEvaluator: texture is False, True (vertex colours) or 'atlas', got {texture!r}")
        self.texture, self.texture_holdout = bool(texture), int(texture_holdout)
        self.texture_atlas, self.texture_res = texture == "atlas", int(texture_res)
        if self.texture_atlas and not L.ATLAS_MIN_RES <= self.texture_res <= L.ATLAS_MAX_RES:
            raise L.GpnerfError(f"MeshEvaluator: texture_res is {L.ATLAS_MIN_RES} to {L.ATLAS_MAX_RES} texels per face edge, got {texture_res!r}")
        if self.texture_holdout < 2:
            raise L.GpnerfError(f"MeshEvaluator: texture_holdout is at least 2 (every texture_holdout-th view is held out), got {texture_holdout!r}")
        self._texture_slots, self._texture_totals, self._texture_frames = [], [], []

    SILHOUETTE_KEYS = ("hull_masks", "hull_Ks", "hull_RTs")

    @property
    def has_mesh_metrics(self):
        """True once a frame with `gt_mesh` (or, with silhouette on, with masks and cameras; or any frame with topology or components on) has been evaluated and not yet summarized
        (evaluate_loop asks)"""
        return (bool(self._slots) or bool(self._sil_slots) or bool(self._topo_slots) or bool(self._vol_slots) or bool(self._comp_slots) or
                bool(self._signed_slots) or bool(self._visible_slots) or bool(self._texture_slots))

    def _padded_lattice(self, axes):
        """(lo, step, dims) of the frame's padded cube lattice in the axes' frame: to_lattice_frame's steps, PAD points around"""
        ax = [np.asarray(a.detach().cpu() if hasattr(a, "detach") else a, dtype=np.float64).reshape(-1) for a in axes]
        step = np.array([(a[-1] - a[0]) / (len(a) - 1) if len(a) > 1 else 1.0 for a in ax])      # to_lattice_frame's
        lo = np.array([a[0] for a in ax]) - self.PAD * step
        return lo, step, tuple(len(a) + 2 * self.PAD for a in ax)

    def _enqueue_signed(self, output, batch):
        from . import frame as F
        if "axes" not in output:
            raise L.GpnerfError("MeshEvaluator(signed=True): the output has no 'axes', so the scan cannot be put on the frame's lattice "
                                "(the inference renderer's render_mesh; the dense renderer's geometry mode returns axes)")
        dev = torch.device(self.metric_device if self.metric_device is not None else "cuda:0")
        lo, step, dims = self._padded_lattice(output["axes"])
        gv, gf = F.mesh_to_device(batch["gt_mesh"], dev)
        scan = F.mesh_sdf(gv, gf, lo, step, dims, self.signed_band * float(step.min()), rule=self.volume_rule)
        pv, pf = F.mesh_to_device(output["mesh"].to_lattice_frame(output["axes"], self.PAD), dev)
        samples = F.sample_surface(pv, pf, self.metric_samples, want_face=False, want_normal=False)["points"]
        # threshold 0: the share of the samples with a value <= 0, i.e. inside the scan; the samples outside the lattice are the NaNs
        self._signed_slots.append(F.distance_stats(scan.sample(samples), thresholds=(0.0,)))
        self._signed_frames.append(self._scalar(batch["frame_index"]))

    def _summarize_signed(self):
        """the signed slots -> (means, per-frame lists), signed_metrics.npy written; resets them"""
        host = torch.stack(self._signed_slots).cpu().numpy()   # the one read
        per_frame = {"signed_mean": [float(h[L.DIST_MEAN]) for h in host], "inside_fraction": [float(h[L.DIST_WITHIN]) for h in host],
                     "signed_outside_lattice": [int(h[L.DIST_NAN]) for h in host]}
        metrics = {k: float(np.mean(v)) for k, v in per_frame.items()}
        per_frame["signed_frame_index"] = list(self._signed_frames)
        table = np.zeros(len(host), dtype=[("frame_index", "i8"), ("samples", "i8"), ("outside_lattice", "i8"), ("signed_mean", "f8"),
                                           ("signed_max", "f8"), ("inside_fraction", "f8")])
        table["frame_index"] = self._signed_frames
        table["samples"], table["outside_lattice"] = host[:, L.DIST_FINITE], host[:, L.DIST_NAN]
        table["signed_mean"], table["signed_max"], table["inside_fraction"] = host[:, L.DIST_MEAN], host[:, L.DIST_MAX], host[:, L.DIST_WITHIN]
        os.makedirs(self.result_path, exist_ok=True)
        np.save(os.path.join(self.result_path, "signed_metrics.npy"), table)        # a structured array: one row per frame
        print(f"signed_mean: {metrics['signed_mean']} (inside_fraction {metrics['inside_fraction']})")
        self._signed_slots, self._signed_frames = [], []
        return metrics, per_frame

    def _enqueue_visible(self, output, batch):
        from . import frame as F
        if "axes" not in output:
            raise L.GpnerfError("MeshEvaluator(visible=True): the output has no 'axes', so its mesh cannot be put into the cameras' frame "
                                "(the inference renderer's render_mesh; the dense renderer's geometry mode returns axes)")
        missing = [k for k in self.SILHOUETTE_KEYS if k not in batch]
        if missing:
            raise L.GpnerfError(f"MeshEvaluator(visible=True): the batch has no {', '.join(repr(k) for k in missing)} (the cameras and masks "
                                "of the dense renderer's geometry mode: hull_masks [1,n,h,w], hull_Ks [1,n,3,3], hull_RTs [1,n,3,4])")
        shape = tuple(batch["hull_masks"].shape)
        if len(shape) != 4:
            raise L.GpnerfError(f"MeshEvaluator(visible=True): hull_masks must be [1,n,h,w], got {shape}")
        dev = torch.device(self.metric_device if self.metric_device is not None else "cuda:0")
        Ks, RTs = F.fetch_host(batch["hull_Ks"][0], batch["hull_RTs"][0])
        rays = F.pixel_rays(Ks, RTs, int(shape[2]), int(shape[3]), device=dev)
        depth = []
        for mesh in (output["mesh"].to_lattice_frame(output["axes"], self.PAD), batch["gt_mesh"]):
            v, f = F.mesh_to_device(mesh, dev)
            grid = F.build_mesh_grid(v, f, cell_cap=self.metric_cell_cap, entry_cap=self.metric_entry_cap, check=False)
            depth.append(F.raycast_mesh(rays, grid=grid)["t"])
        # inf - inf is NaN (neither hit), inf - finite is inf (exactly one): distance_stats counts the three kinds apart
        self._visible_slots.append(F.distance_stats((depth[0] - depth[1]).abs().reshape(-1)))
        self._visible_frames.append(self._scalar(batch["frame_index"]))

    def _summarize_visible(self):
        """the visible-surface slots -> (means, per-frame lists), visible_metrics.npy written; resets them"""
        host = torch.stack(self._visible_slots).cpu().numpy()   # the one read
        both, one, neither = host[:, L.DIST_FINITE], host[:, L.DIST_INF], host[:, L.DIST_NAN]
        with np.errstate(divide="ignore", invalid="ignore"):
            disagreement = one / (both + one)
        per_frame = {"visible_depth_mean": [float(x) for x in host[:, L.DIST_MEAN]],
                     "visible_depth_rms": [float(x) for x in np.sqrt(host[:, L.DIST_MEAN_SQ])],
                     "visible_depth_max": [float(x) for x in host[:, L.DIST_MAX]],
                     "visible_hit_disagreement": [float(x) for x in disagreement]}
        metrics = {k: float(np.max(v) if k == "visible_depth_max" else np.mean(v)) for k, v in per_frame.items()}
        per_frame["visible_frame_index"] = list(self._visible_frames)
        table = np.zeros(len(host), dtype=[("frame_index", "i8"), ("pixels_both", "i8"), ("pixels_one", "i8"), ("pixels_neither", "i8"),
                                           ("depth_mean", "f8"), ("depth_rms", "f8"), ("depth_max", "f8"), ("hit_disagreement", "f8")])
        table["frame_index"] = self._visible_frames
        table["pixels_both"], table["pixels_one"], table["pixels_neither"] = both, one, neither
        table["depth_mean"], table["depth_rms"], table["depth_max"] = host[:, L.DIST_MEAN], np.sqrt(host[:, L.DIST_MEAN_SQ]), host[:, L.DIST_MAX]
        table["hit_disagreement"] = disagreement
        os.makedirs(self.result_path, exist_ok=True)
        np.save(os.path.join(self.result_path, "visible_metrics.npy"), table)       # a structured array: one row per frame
        print(f"visible_depth_mean: {metrics['visible_depth_mean']} (hit disagreement {metrics['visible_hit_disagreement']})")
        self._visible_slots, self._visible_frames = [], []
        return metrics, per_frame

    TEXTURE_KEYS = SILHOUETTE_KEYS + ("hull_imgs",)

    def _enqueue_texture(self, output, batch):
        from . import frame as F
        if "axes" not in output:
            raise L.GpnerfError("MeshEvaluator(texture=True): the output has no 'axes', so its mesh cannot be put into the cameras' frame "
                                "(the inference renderer's render_mesh; the dense renderer's geometry mode returns axes)")
        missing = [k for k in self.TEXTURE_KEYS if k not in batch]
        if missing:
            raise L.GpnerfError(f"MeshEvaluator(texture=True): the batch has no {', '.join(repr(k) for k in missing)} (the cameras, masks and "
                                "images of the hull views: hull_masks [1,n,h,w], hull_Ks [1,n,3,3], hull_RTs [1,n,3,4], hull_imgs [1,n,h,w,3])")
        masks, imgs = torch.as_tensor(batch["hull_masks"][0]), torch.as_tensor(batch["hull_imgs"][0])
        if not masks.is_cuda or not imgs.is_cuda:
            raise L.GpnerfError(f"MeshEvaluator(texture=True): hull_masks and hull_imgs must live on the GPU (got {masks.device}, {imgs.device}); "
                                "no CPU fallback")
        if masks.dtype != torch.uint8 or masks.dim() != 3:
            raise L.GpnerfError(f"MeshEvaluator(texture=True): hull_masks must be uint8 [1,n,h,w] (0, 1, border 100), got {masks.dtype} "
                                f"{tuple(batch['hull_masks'].shape)}")
        if imgs.dtype != torch.float32 or tuple(imgs.shape) != tuple(masks.shape) + (3,):
            raise L.GpnerfError(f"MeshEvaluator(texture=True): hull_imgs must be float32 [1,n,h,w,3] beside hull_masks {tuple(batch['hull_masks'].shape)}, "
                                f"got {imgs.dtype} {tuple(batch['hull_imgs'].shape)}")
        n, h, w = (int(x) for x in masks.shape)
        held = [i for i in range(n) if i % self.texture_holdout == 0][:L.RASTER_MAX_VIEWS]
        source = [i for i in range(n) if i % self.texture_holdout != 0][:L.TEXTURE_MAX_VIEWS]
        if not source:
            raise L.GpnerfError(f"MeshEvaluator(texture=True): {n} hull view(s) leave none to colour from (texture_holdout {self.texture_holdout})")
        Ks, RTs = F.fetch_host(batch["hull_Ks"][0], batch["hull_RTs"][0])
        v, f = F.mesh_to_device(output["mesh"].to_lattice_frame(output["axes"], self.PAD), masks.device)
        grid = F.build_mesh_grid(v, f, cell_cap=self.metric_cell_cap, entry_cap=self.metric_entry_cap, check=False)
        if self.texture_atlas:
            atlas = F.texture_atlas(v, f, Ks[source], RTs[source], imgs[source].contiguous(), res=self.texture_res, grid=grid,
                                    masks=masks[source].contiguous())
            drawn = F.rasterize_mesh(v, f, Ks[held], RTs[held], h, w, want=("face_id",))
            image, totals = atlas.shade(drawn["face_id"], v, f, Ks[held], RTs[held]), atlas.totals
        else:
            tex = F.texture_mesh(v, f, Ks[source], RTs[source], imgs[source].contiguous(), grid=grid, masks=masks[source].contiguous(),
                                 want=("color",))
            drawn = F.rasterize_mesh(v, f, Ks[held], RTs[held], h, w, want=("face_id",), attributes=tex["color"])
            image, totals = drawn["image"], tex["totals"]
        counted = (drawn["face_id"] >= 0) & (masks[held] == 1)
        diff = torch.where(counted[..., None], image - imgs[held], torch.full((), float("nan"), device=masks.device))
        self._texture_slots.append(F.distance_stats(diff.contiguous().reshape(-1)))
        self._texture_totals.append(totals)
        self._texture_frames.append(self._scalar(batch["frame_index"]))

    def _summarize_texture(self):
        """the texture slots -> (means, per-frame lists), texture_metrics.npy written; resets them"""
        host = torch.stack(self._texture_slots).cpu().numpy()   # the two reads
        totals = torch.stack(self._texture_totals).cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            psnr = -10.0 * np.log10(host[:, L.DIST_MEAN_SQ])
            seen = totals[:, 0] / totals.sum(axis=1)
        pixels = (host[:, L.DIST_FINITE] // 3).astype(np.int64)
        per_frame = {"texture_psnr": [float(x) for x in psnr], "texture_pixels": [int(x) for x in pixels],
                     "texture_seen_fraction": [float(x) for x in seen]}
        metrics = {"texture_psnr": float(np.mean(psnr)), "texture_pixels": int(pixels.sum()), "texture_seen_fraction": float(np.mean(seen))}
        per_frame["texture_frame_index"] = list(self._texture_frames)
        table = np.zeros(len(host), dtype=[("frame_index", "i8"), ("pixels", "i8"), ("mean_square", "f8"), ("psnr", "f8"), ("max_abs", "f8"),
                                           ("vertices_seen", "i8"), ("vertices_unseen", "i8")])
        table["frame_index"], table["pixels"], table["mean_square"], table["psnr"] = self._texture_frames, pixels, host[:, L.DIST_MEAN_SQ], psnr
        table["max_abs"] = np.maximum(host[:, L.DIST_MAX], 0.0)
        table["vertices_seen"], table["vertices_unseen"] = totals[:, 0], totals[:, 1]
        os.makedirs(self.result_path, exist_ok=True)
        np.save(os.path.join(self.result_path, "texture_metrics.npy"), table)       # a structured array: one row per frame
        print(f"texture_psnr: {metrics['texture_psnr']} ({metrics['texture_pixels']} pixels, seen fraction {metrics['texture_seen_fraction']})")
        self._texture_slots, self._texture_totals, self._texture_frames = [], [], []
        return metrics, per_frame

    def _enqueue_volume(self, output, batch):
        from . import frame as F
        if "axes" not in output:
            raise L.GpnerfError("MeshEvaluator(volume=True): the output has no 'axes', so the scan cannot be put on the frame's lattice "
                                "(the inference renderer's render_mesh; the dense renderer's geometry mode returns axes)")
        dev = torch.device(self.metric_device if self.metric_device is not None else "cuda:0")
        lo, step, dims = self._padded_lattice(output["axes"])
        pv, pf = F.mesh_to_device(output["mesh"], dev)
        gv, gf = F.mesh_to_device(batch["gt_mesh"], dev)
        pred = F.voxelize_mesh(pv, pf, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims, rule=self.volume_rule)
        gt = F.voxelize_mesh(gv, gf, lo, step, dims, rule=self.volume_rule)
        slot = torch.empty((L.VOXEL_COUNTS + 2,), device=dev, dtype=torch.int64)         # the four counts, then each side's open columns
        F.voxel_stats(pred, gt, out=slot[:L.VOXEL_COUNTS])
        at = L.VOXEL_STATS.index("open_columns")
        slot[L.VOXEL_COUNTS:].copy_(torch.stack([pred.stats[at], gt.stats[at]]))
        self._vol_slots.append(slot)
        self._vol_frames.append(self._scalar(batch["frame_index"]))
        self._vol_cells.append(step.copy())

    def _summarize_volumes(self):
        """the volume slots -> (means, per-frame lists), volume_metrics.npy written; resets them"""
        from . import frame as F
        host = torch.stack(self._vol_slots).cpu().numpy()      # the one read
        rows = [F.read_volume_metrics(h[:L.VOXEL_COUNTS], step) for h, step in zip(host, self._vol_cells)]
        per_frame = {"volume_iou": [r["iou"] for r in rows], "volume_pred": [r["volume_a"] for r in rows], "volume_gt": [r["volume_b"] for r in rows],
                     "volume_precision": [r["precision"] for r in rows], "volume_recall": [r["recall"] for r in rows],
                     "volume_open_columns_pred": [int(h[L.VOXEL_COUNTS]) for h in host],
                     "volume_open_columns_gt": [int(h[L.VOXEL_COUNTS + 1]) for h in host]}
        metrics = {k: float(np.mean(v)) for k, v in per_frame.items()}
        per_frame["volume_frame_index"] = list(self._vol_frames)
        names = ("pred", "gt", "both", "either")
        table = np.zeros(len(rows), dtype=[("frame_index", "i8")] + [(f"points_{k}", "i8") for k in names] +
                         [("open_columns_pred", "i8"), ("open_columns_gt", "i8"), ("cell_volume", "f8")] +
                         [(k, "f8") for k in ("iou", "precision", "recall", "volume_pred", "volume_gt")])
        table["frame_index"] = self._vol_frames
        for i, k in enumerate(names):
            table[f"points_{k}"] = host[:, i]
        table["open_columns_pred"], table["open_columns_gt"] = host[:, L.VOXEL_COUNTS], host[:, L.VOXEL_COUNTS + 1]
        table["cell_volume"] = [float(np.prod(step)) for step in self._vol_cells]
        for k in ("iou", "precision", "recall", "volume_pred", "volume_gt"):
            table[k] = per_frame[f"volume_{k}" if not k.startswith("volume") else k]
        os.makedirs(self.result_path, exist_ok=True)
        np.save(os.path.join(self.result_path, "volume_metrics.npy"), table)        # a structured array: one row per frame
        print(f"volume_iou: {metrics['volume_iou']}")
        for side in ("pred", "gt"):
            if metrics[f"volume_open_columns_{side}"] > 0:
                print(f"volume: the {side} mesh is not closed ({metrics[f'volume_open_columns_' + side]} open columns per frame)")
        self._vol_slots, self._vol_frames, self._vol_cells = [], [], []
        return metrics, per_frame

    def _enqueue_silhouette(self, output, batch):
        from . import frame as F
        if "axes" not in output:
            raise L.GpnerfError("MeshEvaluator(silhouette=True): the output has no 'axes', so its mesh cannot be put into the cameras' frame "
                                "(the inference renderer's render_mesh; the dense renderer's geometry mode returns axes)")
        masks = torch.as_tensor(batch["hull_masks"][0])
        if not masks.is_cuda:
            raise L.GpnerfError(f"MeshEvaluator(silhouette=True): hull_masks must live on the GPU (got {masks.device}); no CPU fallback")
        if masks.dtype != torch.uint8 or masks.dim() != 3:
            raise L.GpnerfError(f"MeshEvaluator(silhouette=True): hull_masks must be uint8 [1,n,h,w] (0, 1, border 100), got {masks.dtype} "
                                f"{tuple(batch['hull_masks'].shape)}")
        masks = masks.contiguous()
        Ks, RTs = F.fetch_host(batch["hull_Ks"][0], batch["hull_RTs"][0])
        pred = output["mesh"].to_lattice_frame(output["axes"], self.PAD)
        v, f = F.mesh_to_device(pred, masks.device)
        drawn = F.rasterize_mesh(v, f, Ks, RTs, int(masks.shape[1]), int(masks.shape[2]), want=("face_id",))
        self._sil_slots.append(F.silhouette_stats(drawn["face_id"], masks))
        self._sil_frames.append(self._scalar(batch["frame_index"]))

    @staticmethod
    def _scalar(v):
        return int(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v).reshape(-1)[0])

    def evaluate(self, output, batch):
        p = self.PAD
        cube = np.asarray(output["cube"])[p:-p, p:-p, p:-p]
        above = cube > self.mesh_th
        if "pts" in batch:
            pts = torch.as_tensor(batch["pts"][0]).detach().cpu().numpy()[above]
        else:
            # the same points from the three axes: pts[i, j, k] = (x[i], y[j], z[k]), without the [X,Y,Z,3] array
            i, j, k = np.nonzero(above)
            ax = [np.asarray(a, dtype=np.float32) for a in output["axes"]]
            pts = np.stack([ax[0][i], ax[1][j], ax[2][k]], axis=-1)
        os.makedirs(self.pts_result_dir, exist_ok=True)
        np.save(os.path.join(self.pts_result_dir, f"{self._scalar(batch['frame_index'])}.npy"), pts)
        if self.export_mesh:
            self.visualize(output, batch)
        if self.repair_gt and batch.get("gt_mesh") is not None:
            # the scan as every metric below sees it: welded, de-duplicated, wound outward (once per frame; the batch itself is left alone)
            from . import frame as F
            gv, gf = F.mesh_to_device(batch["gt_mesh"], torch.device(self.metric_device if self.metric_device is not None else "cuda:0"))
            gv, gf, stats = F.repair_mesh(gv, gf, tol=self.repair_tol)
            batch = {**batch, "gt_mesh": (gv, gf)}
            self._repair_slots.append(stats)
            self._repair_frames.append(self._scalar(batch["frame_index"]))
        if batch.get("gt_mesh") is not None:
            from . import frame as F
            pred = output["mesh"]
            if "axes" in output:
                pred = pred.to_lattice_frame(output["axes"], self.PAD)
            kw = dict(n_samples=self.metric_samples, thresholds=self.metric_thresholds, max_dist=self.metric_max_dist,
                      device=self.metric_device, cell_cap=self.metric_cell_cap, entry_cap=self.metric_entry_cap)
            if self.align is None:
                self._slots.append(F.mesh_metrics(pred, batch["gt_mesh"], **kw))
            else:
                slots, transform = F.mesh_metrics(pred, batch["gt_mesh"], align=self.align, align_iterations=self.align_iterations,
                                                  align_max_dist=self.align_max_dist, want_transform=True, **kw)
                self._slots.append(slots)
                self._transforms.append(transform)
            self._frames.append(self._scalar(batch["frame_index"]))
            if self.volume:
                self._enqueue_volume(output, batch)
            if self.signed:
                self._enqueue_signed(output, batch)
            if self.visible:
                self._enqueue_visible(output, batch)
        if self.silhouette and all(k in batch for k in self.SILHOUETTE_KEYS):
            self._enqueue_silhouette(output, batch)
        if self.texture:
            self._enqueue_texture(output, batch)
        if self.topology:
            from . import frame as F
            v, f = F.mesh_to_device(output["mesh"], torch.device(self.metric_device if self.metric_device is not None else "cuda:0"))
            self._topo_slots.append(F.mesh_topology(f, int(v.shape[0])))
            self._topo_frames.append(self._scalar(batch["frame_index"]))
        if self.components:
            from . import frame as F
            v, f = F.mesh_to_device(output["mesh"], torch.device(self.metric_device if self.metric_device is not None else "cuda:0"))
            comp = F.mesh_components(f, int(v.shape[0]))
            # the largest component's row, picked on the device (row 0 of a table that may have none, when there is no component)
            at = comp.stats[L.COMPONENT_STATS.index("largest")].clamp(min=0).reshape(1)
            boundary = (comp.table.index_select(0, at)[0, L.COMPONENT_COLS.index("boundary_vertices")].reshape(1) if comp.table.shape[0]
                        else torch.zeros((1,), device=v.device, dtype=torch.int64))
            edges = comp.adjacency.stats[[L.TOPOLOGY_STATS.index("nonmanifold_edges"), L.TOPOLOGY_STATS.index("inconsistent_edges")]]
            self._comp_slots.append(torch.cat([comp.stats, boundary, edges]))
            self._comp_frames.append(self._scalar(batch["frame_index"]))

    def _summarize_silhouettes(self):
        """the silhouette slots -> (means, per-frame lists), silhouette_metrics.npy written; resets them"""
        from . import frame as F
        views = {int(s.shape[0]) for s in self._sil_slots}
        host = [s.cpu().numpy() for s in self._sil_slots] if len(views) > 1 else list(torch.stack(self._sil_slots).cpu().numpy())   # the one read
        rows = [F.read_silhouette_metrics(h) for h in host]
        names = ("iou", "precision", "recall")
        per_frame = {f"silhouette_{k}": [r[k] for r in rows] for k in names}
        per_frame["silhouette_frame_index"] = list(self._sil_frames)
        metrics = {f"silhouette_{k}": float(np.mean(per_frame[f"silhouette_{k}"])) for k in names}
        n = max(views)
        table = np.zeros(len(rows), dtype=[("frame_index", "i8"), ("views", "i8")] + [(k, "f8") for k in names] +
                         [(f"{k}_per_view", "f8", (n,)) for k in names] + [("ignored_per_view", "i8", (n,))])
        table["frame_index"], table["views"] = self._sil_frames, [len(r["per_view"]["iou"]) for r in rows]
        for k in names:
            table[k] = [r[k] for r in rows]
            table[f"{k}_per_view"] = np.nan
        for i, r in enumerate(rows):
            for k in names:
                table[f"{k}_per_view"][i, :len(r["per_view"][k])] = r["per_view"][k]
            table["ignored_per_view"][i, :len(r["per_view"]["ignored"])] = r["per_view"]["ignored"]
        os.makedirs(self.result_path, exist_ok=True)
        np.save(os.path.join(self.result_path, "silhouette_metrics.npy"), table)    # a structured array: one row per frame
        for k in names:
            print(f"silhouette_{k}: {metrics['silhouette_' + k]}")
        self._sil_slots, self._sil_frames = [], []
        return metrics, per_frame

    TOPOLOGY_MEANS = ("edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "euler")

    def _summarize_topology(self):
        """the topology slots -> (means, per-frame lists), topology_metrics.npy written; resets them"""
        from . import frame as F
        host = torch.stack(self._topo_slots).cpu().numpy()     # the one read
        rows = [F.read_mesh_topology(h) for h in host]
        per_frame = {f"topology_{k}": [r[k] for r in rows] for k in self.TOPOLOGY_MEANS}
        per_frame["watertight"] = [bool(r["watertight"]) for r in rows]
        per_frame["topology_frame_index"] = list(self._topo_frames)
        metrics = {f"topology_{k}": float(np.mean(per_frame[f"topology_{k}"])) for k in self.TOPOLOGY_MEANS}
        metrics["watertight_frames"] = int(sum(per_frame["watertight"]))
        table = np.zeros(len(rows), dtype=[("frame_index", "i8")] + [(k, "i8") for k in L.TOPOLOGY_STATS] +
                         [(k, "?") for k in ("closed", "oriented", "watertight")])
        table["frame_index"] = self._topo_frames
        for k in table.dtype.names[1:]:
            table[k] = [r[k] for r in rows]
        os.makedirs(self.result_path, exist_ok=True)
        np.save(os.path.join(self.result_path, "topology_metrics.npy"), table)      # a structured array: one row per frame
        print(f"watertight_frames: {metrics['watertight_frames']} of {len(rows)}")
        self._topo_slots, self._topo_frames = [], []
        return metrics, per_frame

    def _summarize_components(self):
        """the component slots -> (means, per-frame lists), components_metrics.npy written; resets them"""
        host = torch.stack(self._comp_slots).cpu().numpy()     # the one read
        n = len(L.COMPONENT_STATS)
        rows = [dict(zip(L.COMPONENT_STATS, (int(x) for x in h[:n]))) for h in host]
        for r, h in zip(rows, host):                           # frame.read_mesh_components' rule, on the largest component's row
            defined = r["largest"] >= 0 and h[n] == 0 and h[n + 1] == 0 and h[n + 2] == 0 and r["largest_euler"] % 2 == 0
            r["largest_genus"] = (2 - r["largest_euler"]) // 2 if defined else -1
        per_frame = {"components": [r["components"] for r in rows], "components_largest_faces": [r["largest_faces"] for r in rows],
                     "components_largest_genus": [r["largest_genus"] for r in rows], "components_frame_index": list(self._comp_frames)}
        metrics = {"components_mean": float(np.mean(per_frame["components"])),
                   "single_component_frames": int(sum(c == 1 for c in per_frame["components"]))}
        table = np.zeros(len(rows), dtype=[("frame_index", "i8")] + [(k, "i8") for k in L.COMPONENT_STATS] + [("largest_genus", "i8")])
        table["frame_index"] = self._comp_frames
        for k in table.dtype.names[1:]:
            table[k] = [r[k] for r in rows]
        os.makedirs(self.result_path, exist_ok=True)
        np.save(os.path.join(self.result_path, "components_metrics.npy"), table)    # a structured array: one row per frame
        print(f"single_component_frames: {metrics['single_component_frames']} of {len(rows)}")
        self._comp_slots, self._comp_frames = [], []
        return metrics, per_frame

    def _summarize_repair(self):
        """the scan repair's slots -> (means, per-frame lists), repair_metrics.npy written; resets them"""
        from . import frame as F
        host = torch.stack(self._repair_slots).cpu().numpy()   # the one read
        rows = [F.read_mesh_repair(h) for h in host]
        per_frame = {f"gt_repair_{k}": [r[k] for r in rows] for k in L.REPAIR_STATS + ("changed",)}
        per_frame["gt_repair_frame_index"] = list(self._repair_frames)
        metrics = {"gt_repaired_frames": int(sum(r["changed"] for r in rows))}
        table = np.zeros(len(rows), dtype=[("frame_index", "i8")] + [(k, "i8") for k in L.REPAIR_STATS] + [("changed", "?")])
        table["frame_index"] = self._repair_frames
        for k in table.dtype.names[1:]:
            table[k] = [r[k] for r in rows]
        os.makedirs(self.result_path, exist_ok=True)
        np.save(os.path.join(self.result_path, "repair_metrics.npy"), table)        # a structured array: one row per frame
        print(f"gt_repaired_frames: {metrics['gt_repaired_frames']} of {len(rows)}")
        self._repair_slots, self._repair_frames = [], []
        return metrics, per_frame

    def summarize(self):
        if (self._sil_slots or self._topo_slots or self._vol_slots or self._comp_slots or self._signed_slots or self._visible_slots or
                self._texture_slots or self._repair_slots):
            parts = (([self._summarize_repair()] if self._repair_slots else []) +
                     ([self._summarize_silhouettes()] if self._sil_slots else []) + ([self._summarize_topology()] if self._topo_slots else []) +
                     ([self._summarize_volumes()] if self._vol_slots else []) + ([self._summarize_components()] if self._comp_slots else []) +
                     ([self._summarize_signed()] if self._signed_slots else []) + ([self._summarize_visible()] if self._visible_slots else []) +
                     ([self._summarize_texture()] if self._texture_slots else []))
            metrics = self._summarize_mesh_metrics() if self._slots else {"per_frame": {}}
            per_frame = metrics.pop("per_frame")
            for means, frames in parts:
                metrics.update(means)
                per_frame.update(frames)
            metrics["per_frame"] = per_frame
            return metrics
        return self._summarize_mesh_metrics()

    def _summarize_mesh_metrics(self):
        if not self._slots:
            return {}
        from . import frame as F
        host = torch.stack(self._slots).cpu().numpy()         # the one read: it waits for the frames' kernels
        moves = [F.read_transform(t) for t in torch.stack(self._transforms).cpu().numpy()] if self._transforms else []
        rows = [F.read_mesh_metrics(s, self.metric_thresholds) for s in host]
        per_frame = {k: [r[k] for r in rows] for k in rows[0]}
        per_frame["frame_index"] = list(self._frames)
        metrics = {k: float(np.mean(v)) for k, v in per_frame.items() if k != "frame_index"}
        if moves:
            aligned = {"align_rms": [m["rms"] for m in moves], "align_rotation_deg": [m["rotation_deg"] for m in moves],
                       "align_translation": [float(np.linalg.norm(m["translation"])) for m in moves]}
            metrics.update({k: float(np.mean(v)) for k, v in aligned.items()})
            aligned["align_status"] = [L.ALIGN_STATUS_NAMES.index(m["status"]) for m in moves]
        table = np.zeros(len(rows), dtype=[(k, "i8" if k == "frame_index" else "f8") for k in ["frame_index"] + list(rows[0])])
        for k in table.dtype.names:
            table[k] = per_frame[k]
        os.makedirs(self.result_path, exist_ok=True)
        np.save(os.path.join(self.result_path, "mesh_metrics.npy"), table)      # a structured array: one row per frame, a field per key
        if moves:
            per_frame.update(aligned)
            np.save(os.path.join(self.result_path, "align_transforms.npy"), np.stack([m["matrix"] for m in moves]))
            self._transforms = []
        for k in ("accuracy", "completeness", "chamfer", "normal_consistency"):
            print(f"{k}: {metrics[k]}")
        metrics["per_frame"] = per_frame
        self._slots, self._frames = [], []
        return metrics

    def visualize(self, output, batch):
        os.makedirs(self.vis_result_dir, exist_ok=True)
        i = self._scalar(batch["frame_index"])
        name = f"{i}_cam{self._scalar(batch['cam_ind'])}.ply" if "cam_ind" in batch else f"{i}.ply"
        output["mesh"].export(os.path.join(self.vis_result_dir, name))


def metrics_switch(device_metrics=None):
    """evaluate_loop's `device_metrics`: None -> the environment's GPNERF_DEVICE_METRICS=1, anything else -> bool(...)"""
    return os.environ.get("GPNERF_DEVICE_METRICS", "0") == "1" if device_metrics is None else bool(device_metrics)


def evaluate_loop(render, eval_loader, cfg, device=None, quiet=False, pipeline=None, device_metrics=None, evaluator=None):
    """`Trainer.evaluate` (libs/trainers/BaseTrainer.py:255-280) without its image writing: for every batch of `eval_loader`
    move it to `device` (`_read_inputs`, :89-97), `ret = render.render(batch)` (the reference calls `.module.render` on its
    DataParallel wrapper; a wrapped model is unwrapped here too), `Evaluator.evaluate(ret, batch)`, `total_time += ret["rtime"]`;
    then `summarize()` when the head renders colour -- or when a MeshEvaluator has been given a `gt_mesh` (its `has_mesh_metrics`).
    Returns {"count", "total_time", "avg_time", "metrics" (summarize()'s dict or None), "mse", "psnr", "ssim" (the per-frame
    lists), "wall_time" (the loop's own clock)} -- the reference prints the average and returns nothing.
    pipeline (not in the reference, whose loop is strictly serial): frame t + 1 is fetched, moved to the device and PREFETCHED
    (Renderer.prefetch: encoder graph, volume builder, frame glue on a second stream) right after frame t's per-ray kernel has been
    enqueued, so the device goes from one frame's per-ray kernel straight into the next frame's producers while the host evaluates
    frame t.  Default: on when the renderer offers `prefetch` and is neither progressive nor sharded.  Same bits per frame.
    device_metrics (not in the reference): the frames' metrics by `DeviceEvaluator` -- enqueued behind each frame's per-ray kernel,
    read once behind the last frame (inside `wall_time`).  Default (None): on with GPNERF_DEVICE_METRICS=1 in the environment,
    otherwise off.
    evaluator (not in the reference, whose Trainer.evaluate always constructs the image Evaluator, BaseTrainer.py:257, and imports
    the mesh one without using it): an instance used in place of the one constructed here -- a MeshEvaluator for a geometry-mode
    renderer, whose output has no rgb_map.  Without it the loop builds what it always built, whatever use_rgbhead says.  The
    per-frame lists are the evaluator's where it has them, otherwise empty.  A renderer whose head has use_rgbhead False has no
    per-ray kernel to prefetch behind: `pipeline` defaults to off for it."""
    model = getattr(render, "module", render)
    model.eval()
    if evaluator is None:
        evaluator = (DeviceEvaluator if metrics_switch(device_metrics) else Evaluator)(cfg, cfg.test.test_seq)
    count, total_time = 0, 0.0
    if pipeline is None:
        pipeline = (hasattr(model, "prefetch") and not getattr(model, "progressive", False) and getattr(model, "shard_group", None) is None
                    and getattr(getattr(model, "nerfhead", None), "use_rgbhead", True))

    def move(v):
        if device is None:
            return v
        to = lambda b: b.to(device) if hasattr(b, "to") else b   # (a batch's gt_mesh -- a mesh.Mesh or numpy arrays -- stays; mesh_metrics uploads it)
        if isinstance(v, (list, tuple)):
            return [to(b) for b in v]
        if isinstance(v, dict):
            return {k: to(b) for k, b in v.items()}
        return to(v)

    import time as _time
    t_loop = _time.time()
    if not pipeline:
        for data in eval_loader:
            with torch.no_grad():
                val = {k: move(v) for k, v in data.items()}
                ret = model.render(val)
                evaluator.evaluate(ret, val)
            total_time += ret["rtime"]                       # the dense renderer of the reference returns no "rtime": KeyError there
            count += 1
    else:
        it = iter(eval_loader)

        def fetch():
            data = next(it, None)
            if data is None:
                return None
            val = {k: move(v) for k, v in data.items()}
            if hasattr(model, "host_consts"):
                # the frame's small constants go to the host NOW, from the loader's CPU tensors when it hands out those (no copy at
                # all), otherwise while no per-ray kernel is running: inside prefetch() the copy would wait for that kernel
                src = data if all(not (isinstance(v, torch.Tensor) and v.is_cuda) for v in data.values()) else val
                val["_gpnerf_consts"] = model.host_consts(src)
            return val

        with torch.no_grad():
            val = fetch()
            pre = model.prefetch(val) if val is not None else None
            while val is not None:
                nxt = fetch()
                ret = model.render(val, prefetched=pre, next_batch=nxt)
                pre = ret.pop("next_prefetched", None)
                evaluator.evaluate(ret, val)
                total_time += ret["rtime"]
                count += 1
                val = nxt
    per_frame = {k: list(getattr(evaluator, k, ())) for k in ("mse", "psnr", "ssim")}
    wall = _time.time() - t_loop                              # (behind the lists: the device evaluator's one read belongs to the loop)
    # the reference summarizes when the head renders colour; a MeshEvaluator that has seen a gt_mesh has numbers too
    wants = cfg.head.rgb.use_rgbhead or getattr(evaluator, "has_mesh_metrics", False)
    if quiet:                                                 # (summarize() prints its means, as the reference's does)
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            metrics = evaluator.summarize() if wants else None
    else:
        metrics = evaluator.summarize() if wants else None
    if not quiet:
        print(f"avg total render time: {total_time / max(count, 1)}s per sample")
    return dict(count=count, total_time=total_time, avg_time=total_time / max(count, 1), metrics=metrics, wall_time=wall, **per_frame)
