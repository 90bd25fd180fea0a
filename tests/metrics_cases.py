"""What the device-metrics tests share: the scipy restatement of the SSIM definition and the ragged-mask case of
tests/test_evaluator.py (copies: that file is the torch path's own yardstick), the masks the device path is held to, and the
yardstick itself -- the torch `Evaluator` on CPU float64 tensors."""
import importlib
import types

import numpy as np
import torch
from scipy.ndimage import uniform_filter

ev = importlib.import_module("gp-nerf_amd.evaluator")


def ssim_restated(a, b):
    """compare_ssim(a, b, multichannel=True), float64 images -> data_range 2, win 7, sample covariance, crop 3."""
    vals = []
    for c in range(a.shape[2]):
        x, y = a[..., c].astype(np.float64), b[..., c].astype(np.float64)
        ux, uy = uniform_filter(x, 7), uniform_filter(y, 7)
        n = 49.0 / 48.0
        vx, vy = n * (uniform_filter(x * x, 7) - ux * ux), n * (uniform_filter(y * y, 7) - uy * uy)
        vxy = n * (uniform_filter(x * y, 7) - ux * uy)
        c1, c2 = (0.01 * 2) ** 2, (0.03 * 2) ** 2
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        vals.append(s[3:-3, 3:-3].mean())
    return float(np.mean(vals))


def cfg_of(H, W):
    return types.SimpleNamespace(dataset=types.SimpleNamespace(H=H * 2, W=W * 2, ratio=0.5))


def colours(mask, seed):
    """gt uniform in [0, 1), pred = clip(gt + 0.05 noise), float32 [n, 3] for the mask's n pixels"""
    g = np.random.Generator(np.random.PCG64(seed))
    n = int(mask.sum())
    gt = g.uniform(0, 1, (n, 3)).astype(np.float32)
    pred = np.clip(gt + 0.05 * g.standard_normal((n, 3)).astype(np.float32), 0, 1).astype(np.float32)
    return pred, gt


def _case(H=40, W=56, seed=0):
    """tests/test_evaluator.py's case: a ragged 80 % mask inside rows 6..30, columns 9..43"""
    g = np.random.Generator(np.random.PCG64(seed))
    mask = np.zeros((H, W), bool)
    mask[6:31, 9:44] = g.uniform(size=(25, 35)) < 0.8
    mask[6, 9] = mask[30, 43] = True
    n = int(mask.sum())
    gt = g.uniform(0, 1, (n, 3)).astype(np.float32)
    pred = np.clip(gt + 0.05 * g.standard_normal((n, 3)).astype(np.float32), 0, 1)
    cfg = types.SimpleNamespace(dataset=types.SimpleNamespace(H=H * 2, W=W * 2, ratio=0.5))
    batch = {"mask_at_box": torch.from_numpy(mask.reshape(1, -1)), "rgb": torch.from_numpy(gt)[None]}
    return cfg, batch, mask, pred, gt


def ragged(H, W, y0, y1, x0, x1, seed, fill=0.8):
    """a ragged mask whose bounding rectangle is rows y0..y1, columns x0..x1 (inclusive)"""
    g = np.random.Generator(np.random.PCG64(seed))
    mask = np.zeros((H, W), bool)
    mask[y0:y1 + 1, x0:x1 + 1] = g.uniform(size=(y1 - y0 + 1, x1 - x0 + 1)) < fill
    mask[y0, x0] = mask[y1, x1] = mask[y0, x1] = mask[y1, x0] = True
    return mask


def rect_of(mask):
    ys, xs = np.nonzero(mask)
    return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)) if len(ys) else (0, 0, 0, 0)


def yardstick(mask, pred, gt):
    """(mse, psnr, ssim) of the torch `Evaluator` on CPU float64 tensors, and the scipy restatement's SSIM on the same crop"""
    H, W = mask.shape
    e = ev.Evaluator(cfg_of(H, W), "ref")
    batch = {"mask_at_box": torch.from_numpy(mask.reshape(1, -1)), "rgb": torch.from_numpy(gt).double()[None]}
    e.evaluate({"rgb_map": torch.from_numpy(pred).double()[None]}, batch)
    a, b = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    a[mask], b[mask] = pred, gt
    x, y, w, h = rect_of(mask)
    return e.mse[0], e.psnr[0], e.ssim[0], ssim_restated(a[y:y + h, x:x + w], b[y:y + h, x:x + w])
