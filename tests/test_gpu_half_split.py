"""GPU: the fused render kernels divide each view's per-ray arithmetic between a tile's two lane halves (gp-nerf_amd/csrc/
gpnerf_kernels.hip view_axes_halved: x in half 0, y in half 1, exchanged with v_permlane32_swap) -- held to the CPU oracle on inputs on
which an x / y mix-up cannot hide, at the tolerances tests/test_gpu_plans.py against_the_oracle uses.

Two scenes with non-square sources (40 x 72 and 72 x 40 images, 10 x 18 and 18 x 10 feature maps; every volume level has three
different extents), random pose, S = 16, 2 880 base rays each.  Before any GPU call the oracle's own stage vectors say that the inputs
bite: a good part of the (sample, view) pairs fall outside their view, a good part of the samples have exactly one grid coordinate
outside [-1, 1], and enough weights are non-zero for the colour branch to matter.

Every kernel that takes the halved path is rendered: the base rays once (STATIC: the colour passes of the wavefront), the base rays
repeated modulo the frame to the smallest ragged ray count whose plan on this device is QUEUE + UNIFIED (the headline's kernel), the
same count with shared_device=True (LIST: colour_units_kernel), the scene with camera space negated under neg_ray (the flipped
order), and the folded form.  Each plan is asserted before its render."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_gpu_plans.py TOL: max-abs on the maps against the reference CPU path
S = 16
KEYS = ("rgb_map", "depth_map", "acc_map", "weights", "rgb_in_map")
SCENES = {"wide": dict(H=40, W=72, seed=3, fill="full", pose="random"), "tall": dict(H=72, W=40, seed=4, fill="full", pose="random")}


@pytest.fixture(scope="module")
def fm():
    return importlib.import_module("gp-nerf_amd.frame")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def build_frame(fm, sc):
    return fm.Frame(to_dev(sc["src_imgs"][0]), to_dev(sc["featmaps"]), [to_dev(v) for v in sc["volumes"]], to_dev(sc["src_Ks"][0]),
                    to_dev(sc["src_poses"][0]), sc["Rh"][0], sc["Th"][0], sc["bounds"][0, 0], sc["voxel_size"], sc["out_sh"][0],
                    fm.pack_head(sc["head"], torch.device("cuda:0")))


class Case:
    """one scene: its oracle renders (forward with the stage vectors, and camera space negated under neg_ray), checked for the
    conditions above on the host; frames on the device are built where a test first asks"""

    def __init__(self, fm, syn, oracle, name):
        self.fm, self.name = fm, name
        kw = SCENES[name]
        self.sc, self.sc_neg = syn.make_scene(**kw), syn.make_scene(neg_cams=True, **kw)
        self.rays_h = oracle.rays_of(self.sc)
        assert self.rays_h.shape[0] == 2880 and np.array_equal(self.rays_h, oracle.rays_of(self.sc_neg))
        H, W = kw["H"], kw["W"]
        assert self.sc["src_imgs"][0].shape[-2:] == (H, W) or self.sc["src_imgs"][0].shape[1:3] == (H, W), self.sc["src_imgs"][0].shape
        assert all(len(set(v.shape[-3:])) == 3 for v in self.sc["volumes"]), [v.shape for v in self.sc["volumes"]]
        self.ref = oracle.render(self.sc, S, stages=True)
        self.ref_neg = oracle.render(self.sc_neg, S, neg_ray=True)
        invalid = float((self.ref["st_mask"] == 0).mean())
        outside = (np.abs(self.ref["st_grid"]) > 1.0).sum(-1)
        one_axis = float((outside == 1).mean())
        nonzero = float((self.ref["weights"] != 0).mean())
        per_view = [round(float((self.ref["st_mask"][..., v] == 0).mean()), 4) for v in range(self.ref["st_mask"].shape[-1])]
        print(f"\n  {name}: {invalid:.4f} of the (sample, view) pairs are outside their view (per view {per_view}), {one_axis:.4f} of the "
              f"samples have exactly one grid coordinate outside [-1, 1], {nonzero:.4f} of the weights are non-zero")
        assert invalid >= 0.05 and one_axis >= 0.20 and nonzero >= 0.30, (name, invalid, one_axis, nonzero)
        assert float((self.ref_neg["weights"] != 0).mean()) >= 0.30
        self._dev = {}

    def on_device(self, neg=False):
        if neg not in self._dev:
            self._dev[neg] = (build_frame(self.fm, self.sc_neg if neg else self.sc), to_dev(self.rays_h))
        return self._dev[neg]

    def queue_rays(self):
        """the smallest ragged ray count (whole tiles + 17 rays) whose plan on this device is QUEUE + UNIFIED"""
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        for tiles in range(1, 4 * cus * 8 + 1):
            n = tiles * 32 + 17
            if self.fm.render_plan(None, n, S, n_cus=cus).triple()[:2] == ("QUEUE", "UNIFIED"):
                return n
        pytest.fail(f"no ray count up to four rounds of wavefronts gets QUEUE + UNIFIED on {cus} CUs")

    def check(self, n, want_plan, neg=False, **kw):
        fr, base = self.on_device(neg)
        if neg:
            kw["neg_ray"] = True
        plan = self.fm.render_plan(None, n, S, **kw)
        print(f"\n  {self.name}: n_rays={n} S={S} {kw} -> {plan}")
        t = plan.triple()
        assert all(w is None or w == g for w, g in zip(want_plan, t)), (want_plan, t)
        rays = base[torch.arange(n, device=base.device) % base.shape[0]].contiguous()
        got = {k: v.cpu().numpy() for k, v in self.fm.render_fused(fr, rays, S, **kw).items()}
        ref = self.ref_neg if neg else self.ref
        rows = np.arange(n) % base.shape[0]
        for k in KEYS:
            err = float(np.abs(got[k] - ref[k][rows]).max())
            print(f"    {k}: max error against the oracle {err:.3g}")
            assert err < TOL, (k, err, str(plan))
        err = float(np.abs(got["z_vals"] - ref["z_vals"][rows]).max())
        print(f"    z_vals: max error against the oracle {err:.3g}")
        assert err <= 1e-6, ("z_vals", err, str(plan))
        assert np.array_equal(got["ray_mask"].astype(bool), ref["ray_mask"][rows].astype(bool)), str(plan)
        return plan


_CASES = {}


@pytest.fixture(params=list(SCENES))
def case(request, fm, syn, oracle):
    if request.param not in _CASES:
        _CASES[request.param] = Case(fm, syn, oracle, request.param)
    return _CASES[request.param]


def test_the_base_rays_with_the_colour_passes_of_the_wavefront(case):
    plan = case.check(case.rays_h.shape[0], ("STATIC", "WAVE", "REF"))
    assert plan.split > 1


def test_the_unified_launch(case):
    case.check(case.queue_rays(), ("QUEUE", "UNIFIED", "REF"))


def test_the_list_launch_and_its_own_kernel(case):
    case.check(case.queue_rays(), (None, "LIST", "REF"), shared_device=True)


def test_camera_space_negated_in_the_flipped_order(case):
    case.check(case.queue_rays(), ("QUEUE", "UNIFIED", "REF"), neg=True)


def test_the_folded_form(case):
    case.check(case.queue_rays(), ("QUEUE", None, "FOLD"), fold=True)
