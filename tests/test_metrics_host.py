"""CPU: the host pieces of the device evaluator (gpnerf_image_metrics, evaluator.DeviceEvaluator) -- the workspace size, the entry
point's argument checks, the refusal of CPU tensors, evaluate_loop's switch, and that the plain Evaluator does not look at it."""
import ctypes as C
import importlib
import re
import os
import types

import pytest
import torch

import metrics_cases as mcs

ev = importlib.import_module("gp-nerf_amd.evaluator")
L = importlib.import_module("gp-nerf_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_bytes_is_host_arithmetic():
    ws = L.lib().gpnerf_metrics_workspace_bytes
    sizes = [1, 6, 7, 8, 38, 39, 63, 64, 65, 512, 513, 1024]
    for h in sizes:
        for w in sizes:
            b = int(ws(h, w))
            assert b > 0 and b % 256 == 0, (h, w, b)
    for a, b in zip(sizes, sizes[1:]):
        for o in sizes:
            assert ws(a, o) <= ws(b, o) and ws(o, a) <= ws(o, b), (a, b, o)
    assert ws(512, 512) < 1 << 20                      # mask words and partial sums, no dense image
    assert ws(0, 8) == 0 and ws(8, 0) == 0 and ws(-1, 8) == 0 and ws(1 << 16, 1 << 16) == 0      # dims the call refuses


def test_image_metrics_rejects_bad_arguments_on_the_host():
    lib = L.lib()
    H, W = 40, 56
    need = int(lib.gpnerf_metrics_workspace_bytes(H, W))

    def call(pred=0x1000, gt=0x1000, mask=0x1000, H=H, W=W, n=100, ws=0x1000, ws_bytes=need, out=0x1000):
        return lib.gpnerf_image_metrics(pred, gt, mask, H, W, n, ws, ws_bytes, out, None)

    for name in ("pred", "gt", "mask", "ws", "out"):
        assert call(**{name: None}) == -1, name
    assert call(H=0) == -1 and call(H=-3) == -1
    assert call(W=0) == -1 and call(W=-3) == -1
    assert call(n=-1) == -1
    assert call(n=H * W + 1) == -1
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1
    assert call(H=1 << 16, W=1 << 16, ws_bytes=1 << 40) == -1                 # H * W beyond the 31-bit pixel ranks
    assert lib.gpnerf_strerror(-1) == b"invalid argument"


def test_the_slot_layout_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "gpnerf_hip.h")).read()
    for name in ("MSE", "SSIM", "X", "Y", "W", "H", "POPULATION", "STATUS", "DOUBLES"):
        assert re.search(rf"#define GPNERF_METRICS_{name} {getattr(L, 'METRICS_' + name)}\b", hdr), name


def test_device_evaluator_refuses_cpu_tensors():
    cfg, batch, mask, pred, gt = mcs._case()
    e = ev.DeviceEvaluator(cfg, "seq")
    with pytest.raises(ValueError, match="CPU tensor"):
        e.evaluate({"rgb_map": torch.from_numpy(pred)[None]}, batch)
    assert e.mse == [] and e.psnr == [] and e.ssim == []


def test_device_evaluator_keeps_the_torch_path_for_pred_img():
    """an output with `pred_img` (host arrays by the progressive renderer's contract) is the inherited path's, also on the CPU"""
    import numpy as np
    cfg, batch, mask, pred, gt = mcs._case(seed=3)
    img = np.zeros(mask.shape + (3,), np.float32)
    img[mask] = pred
    a, b = ev.Evaluator(cfg, "s"), ev.DeviceEvaluator(cfg, "s")
    a.evaluate({"pred_img": img}, batch)
    b.evaluate({"pred_img": img}, batch)
    assert a.mse == b.mse and a.psnr == b.psnr and a.ssim == b.ssim and len(b.mse) == 1
    assert a.summarize() == b.summarize() and b.mse == [] and b.psnr == [] and b.ssim == []


def test_the_loops_switch_reads_the_variable_only_for_none(monkeypatch):
    monkeypatch.delenv("GPNERF_DEVICE_METRICS", raising=False)
    assert ev.metrics_switch() is False and ev.metrics_switch(None) is False
    assert ev.metrics_switch(True) is True and ev.metrics_switch(1) is True and ev.metrics_switch(False) is False
    monkeypatch.setenv("GPNERF_DEVICE_METRICS", "1")
    assert ev.metrics_switch(None) is True
    assert ev.metrics_switch(False) is False and ev.metrics_switch(0) is False and ev.metrics_switch(True) is True
    monkeypatch.setenv("GPNERF_DEVICE_METRICS", "0")
    assert ev.metrics_switch(None) is False and ev.metrics_switch(True) is True
    # ... and the loop itself takes its evaluator by it: an empty loader shows which class it built
    made = []

    class Spy(ev.Evaluator):
        def __init__(self, *a):
            made.append(type(self).__name__)
            super().__init__(*a)

    class SpyDevice(Spy):
        pass

    monkeypatch.setattr(ev, "Evaluator", Spy)
    monkeypatch.setattr(ev, "DeviceEvaluator", SpyDevice)
    cfg = types.SimpleNamespace(test=types.SimpleNamespace(test_seq="s"), head=types.SimpleNamespace(rgb=types.SimpleNamespace(use_rgbhead=False)))
    model = torch.nn.Identity()
    for env, arg, want in (("0", None, "Spy"), ("1", None, "SpyDevice"), ("1", False, "Spy"), ("0", True, "SpyDevice")):
        monkeypatch.setenv("GPNERF_DEVICE_METRICS", env)
        out = ev.evaluate_loop(model, [], cfg, quiet=True, pipeline=False, device_metrics=arg)
        assert made[-1] == want and out["count"] == 0 and out["mse"] == [], (env, arg)
    monkeypatch.delenv("GPNERF_DEVICE_METRICS")
    ev.evaluate_loop(model, [], cfg, quiet=True, pipeline=False)
    assert made[-1] == "Spy"


def test_the_plain_evaluator_does_not_look_at_the_variable(monkeypatch):
    cfg, batch, mask, pred, gt = mcs._case()
    got = []
    for env in (None, "1", "0"):
        if env is None:
            monkeypatch.delenv("GPNERF_DEVICE_METRICS", raising=False)
        else:
            monkeypatch.setenv("GPNERF_DEVICE_METRICS", env)
        e = ev.Evaluator(cfg, "seq")
        e.evaluate({"rgb_map": torch.from_numpy(pred)[None]}, batch)
        got.append((e.mse[0], e.psnr[0], e.ssim[0]))
    assert got[0] == got[1] == got[2]
    assert abs(got[0][2] - mcs.yardstick(mask, pred, gt)[3]) < 1e-9
