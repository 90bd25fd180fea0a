"""GPU: the HIP path (through the C ABI) against the golden vectors and the CPU oracle."""
import importlib

import numpy as np
import pytest
import torch

from golden_cases import (FAST_FORM_K, assert_close, case_names, demo_case_names, demo_tolerances, load, rays_case_names, scene_of, trained_case_names,
                          trained_tolerance)

pytestmark = pytest.mark.gpu

# north_star: within 1e-4 max-abs of the reference on RGB / depth
TOL = 1e-4
# what the kernels actually deliver on the initialisation-scale golden cases since the geometry runs in the reference's summation
# order (round 4): rgb <= 1.6e-6, depth <= 8e-6 (tools/parity_report.py); a regression bound well inside north_star's
TIGHT = 2e-5


@pytest.fixture(scope="module")
def fm():
    return importlib.import_module("gp-nerf_amd.frame")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def build_frame(fm, sc):
    blob = fm.pack_head(sc["head"], torch.device("cuda:0"))
    return fm.Frame(to_dev(sc["src_imgs"][0]), to_dev(sc["featmaps"]), [to_dev(v) for v in sc["volumes"]],
                    to_dev(sc["src_Ks"][0]), to_dev(sc["src_poses"][0]), sc["Rh"][0], sc["Th"][0], sc["bounds"][0, 0],
                    sc["voxel_size"], sc["out_sh"][0], blob)


def rays_of(sc):
    return to_dev(np.concatenate([sc["ray_o"][0], sc["ray_d"][0], sc["near"][0][:, None], sc["far"][0][:, None]], 1))


def cpu(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize("name", case_names())
def test_fused_matches_reference_golden(name, fm):
    z, meta = load(name)
    sc = scene_of(meta)
    S = meta["n_samples"]
    fr = build_frame(fm, sc)
    got = cpu(fm.render_fused(fr, rays_of(sc), S, neg_ray=meta["neg_ray"], want=("weights", "z_vals", "rgb_in", "ray_mask", "raw")))
    assert_close(got["rgb_map"], z["rgb_map"], TIGHT, "rgb_map")
    assert_close(got["depth_map"], z["depth_map"], TIGHT, "depth_map")
    assert_close(got["acc_map"], z["acc_map"], TIGHT, "acc_map")
    assert_close(got["rgb_in_map"], z["rgb_in_map"], TIGHT, "rgb_in_map")
    assert_close(got["disp_map"], z["disp_map"], 5e-4, "disp_map")
    if "weights" in z:
        assert_close(got["weights"], z["weights"], TOL, "weights")
        assert_close(got["z_vals"], z["z_vals"], 1e-6, "z_vals")
    if "st_raw" in z:
        idx = z["st_rays"]
        assert_close(got["raw"][idx], z["st_raw"], TOL, "raw")
        assert np.array_equal(got["ray_mask"][idx].astype(bool), z["st_ray_mask"])


@pytest.mark.parametrize("form", ["fp32_reference_order", "fp32_folded", "split_f16"])
@pytest.mark.parametrize("name", trained_case_names())
def test_fused_on_trained_like_parameters(name, form, fm, oracle):
    """Parity on something other than `weights_init` parameters -- head weights x 1 / 1.5 / 2 / 3 with non-zero biases, feature maps
    and volumes x 4 with log-normal tails, ReLU-sparse levels, >= 4 096 rays x 64 samples, produced by the reference's Renderer.render.
    Every kernel form against (a) the reference's float32 maps and (b) the maps of its head evaluated in float64.
    The DEFAULT form (reference summation order, round 5) is held to 2 x the C ORACLE's own distance from the reference on every
    map (the oracle follows the reference op for op) and to golden_cases.trained_tolerance (k = 2: 1e-4 where
    float32 can deliver it, 2 x the reference's own float32-vs-float64 noise beyond).  The two fast forms (`hip_render_fold`,
    `hip_render_fast`) round in another order and are held to k = FAST_FORM_K.  tools/trained_like_report.py prints the table;
    oracle/kernel_order.inc attributes the difference deviation by deviation."""
    z, meta = load(name)
    sc = scene_of(meta)
    S = meta["n_samples"]
    fr = build_frame(fm, sc)
    kw = {"fp32_reference_order": dict(), "fp32_folded": dict(fold=True), "split_f16": dict(split_f16=True)}[form]
    k_tol = 2.0 if form == "fp32_reference_order" else FAST_FORM_K
    got = cpu(fm.render_fused(fr, rays_of(sc), S, want=("weights", "z_vals", "rgb_in", "guard_tiles") if form == "split_f16" else ("weights", "z_vals", "rgb_in"), **kw))
    ref = oracle.render(sc, S)
    line = []
    for k in ("rgb_map", "depth_map", "acc_map", "rgb_in_map"):
        err = assert_close(got[k], z[k], trained_tolerance(z, k, k=k_tol), f"{name} {k}")
        err_o = float(np.abs(ref[k].astype(np.float64) - z[k]).max())
        line.append(f"{k} {err:.2e} (oracle {err_o:.2e}, reference's own {float(z['spread_' + k]):.2e})")
        if form == "fp32_reference_order":
            assert err <= 2.0 * err_o + 1e-6, f"{name} {k}: {err:.2e} is more than twice the op-for-op oracle's distance {err_o:.2e}"
    if form == "fp32_reference_order" and "h1p5" in name:
        assert float(np.abs(got["depth_map"].astype(np.float64) - z["depth_map"]).max()) <= 1e-4
    for k in ("rgb_map", "depth_map", "acc_map"):
        assert_close(got[k].astype(np.float64), z[k + "_head64"], trained_tolerance(z, k, k=k_tol), f"{name} {k} vs the float64 head")
    if "weights" in z:
        assert_close(got["weights"], z["weights"], max(trained_tolerance(z, k, k=k_tol) for k in ("rgb_map", "acc_map")), "weights")
        assert_close(got["z_vals"], z["z_vals"], 1e-6, "z_vals")
    print(f"{name} [{form}]: " + "; ".join(line) + (f"; guard tiles {int(got['guard_tiles'][0])}" if "guard_tiles" in got else ""))


def test_reference_order_form_is_its_cpu_twin(fm, oracle):
    """oracle/kernel_order.inc restates the reference-order form's arithmetic on the CPU (everything but v_exp_f32's last bit): the
    kernel and its twin must be the same distance from the reference (that is what makes the twin's deviation-by-deviation
    attribution evidence about the KERNEL), and within rounding of each other."""
    name = "trained_h1p5_s64"
    z, meta = load(name)
    sc = scene_of(meta)
    S = meta["n_samples"]
    got = cpu(fm.render_fused(build_frame(fm, sc), rays_of(sc), S))
    with oracle.kernel_order(oracle.KO_KERNEL_REF):
        twin = oracle.render(sc, S, want_weights=False)
    for k in ("rgb_map", "depth_map", "acc_map"):
        d_hip = float(np.abs(got[k].astype(np.float64) - z[k]).max())
        d_twin = float(np.abs(twin[k].astype(np.float64) - z[k]).max())
        assert abs(d_hip - d_twin) <= 0.25 * d_twin + 1e-6, (k, d_hip, d_twin)
        assert_close(got[k], twin[k], 3e-5, f"{k}: kernel vs its CPU twin")


@pytest.mark.parametrize("split_f16", [False, True])
@pytest.mark.parametrize("S,n_rays", [(1, 5), (2, 33), (7, 31), (64, 100), (128, 64)])
def test_fused_matches_oracle_ragged(S, n_rays, split_f16, fm, oracle, syn):
    sc = syn.make_scene(H=16, W=16, seed=100 + S, fill="full", pose="random", aabb_half=(0.12, 0.16, 0.05), bias_std=0.1,
                        max_rays=n_rays)
    fr = build_frame(fm, sc)
    got = cpu(fm.render_fused(fr, rays_of(sc), S, want=("weights", "z_vals", "rgb_in", "ray_mask", "raw"), split_f16=split_f16))
    ref = oracle.render(sc, S, stages=True)
    for k in ("rgb_map", "depth_map", "acc_map", "rgb_in_map", "weights"):
        assert_close(got[k], ref[k], TOL, k)
    assert_close(got["z_vals"], ref["z_vals"], 1e-6, "z_vals")
    assert_close(got["raw"], ref["st_raw"], TOL, "raw")
    assert np.array_equal(got["ray_mask"], ref["ray_mask"])


def test_empty_ray_list(fm, syn):
    sc = syn.make_scene(H=8, W=8, seed=1, aabb_half=(0.12, 0.16, 0.05))
    fr = build_frame(fm, sc)
    got = fm.render_fused(fr, torch.empty((0, 8), device="cuda:0"), 8)
    assert got["rgb_map"].shape == (0, 3)


def test_head_forward_matches_oracle(fm, oracle, syn):
    sc = syn.make_scene(H=16, W=16, seed=9, fill="full", pose="random", aabb_half=(0.12, 0.16, 0.05), bias_std=0.1, max_rays=70)
    S = 8
    ref = oracle.render(sc, S, stages=True)
    blob = fm.pack_head(sc["head"], torch.device("cuda:0"))
    raw = fm.head_forward(blob, to_dev(ref["st_vol_feat"].reshape(-1, 128)), to_dev(ref["st_rgb_feat"].reshape(-1, 3, 35)),
                          to_dev(ref["st_mask"].reshape(-1, 3))).cpu().numpy()
    assert_close(raw, ref["st_raw"].reshape(-1, 4), TOL, "raw")


def test_composite_matches_oracle(fm, oracle):
    g = np.random.Generator(np.random.PCG64(5))
    N, S = 77, 40
    raw = g.random((N, S, 4), dtype=np.float32)
    raw[..., 3] = np.maximum(g.standard_normal((N, S), dtype=np.float32), 0) * 2
    raw[:3, :, 3] = 0  # acc == 0 -> disp NaN
    z = np.sort(g.random((N, S), dtype=np.float32) * 2 + 2, axis=1)
    nvalid = g.integers(0, 4, (N, S)).astype(np.float32)
    for neg in (False, True):
        got = cpu(fm.composite(to_dev(raw), to_dev(z), to_dev(nvalid), neg=neg))
        ref = oracle.composite(raw, z, nvalid, neg=neg)
        for k in ("rgb_map", "depth_map", "acc_map", "weights"):
            assert_close(got[k], ref[k], 1e-5, k)
        assert_close(got["disp_map"], ref["disp_map"], 1e-4, "disp")
        assert np.array_equal(got["ray_mask"].astype(bool), ref["ray_mask"])


@pytest.mark.parametrize("name", rays_case_names())
def test_make_rays_matches_reference_golden(name, fm, syn):
    """gpnerf_make_rays against numpy's run of get_rays + get_near_far (three 512x512 cameras incl. the +1e-5 clamp and
    rays through the box edge): mask_at_box, rays, near, far bit-exact."""
    import os
    from golden_cases import GOLDEN_DIR
    from test_oracle_golden import check_rays_against_golden
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    K, R, T, bounds = syn.make_ray_camera(bytes(z["kind"]).decode(), int(z["H"]), int(z["W"]))
    rays, mask = fm.make_rays(int(z["H"]), int(z["W"]), K, R, T, bounds, torch.device("cuda:0"))
    rays, mask = rays.cpu().numpy(), mask.cpu().numpy()
    check_rays_against_golden(z, rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7], mask)


def test_early_termination_stays_within_bound(fm, oracle, syn):
    sc = syn.make_scene(H=16, W=16, seed=21, fill="full", pose="identity", aabb_half=(0.12, 0.16, 0.05), sigma_bias=1.0)
    S = 64
    fr = build_frame(fm, sc)
    full = cpu(fm.render_fused(fr, rays_of(sc), S))
    cut = cpu(fm.render_fused(fr, rays_of(sc), S, early_term=True, term_eps=1e-5))
    # stopping at T < eps leaves rgb/acc within eps and depth within eps * far
    assert_close(cut["rgb_map"], full["rgb_map"], 2e-5, "rgb (early term)")
    assert_close(cut["depth_map"], full["depth_map"], 1e-4, "depth (early term)")
    assert (cut["weights"] == 0).sum() > (full["weights"] == 0).sum(), "no sample was skipped: the test scene is not opaque enough"


@pytest.mark.parametrize("name", ["base_s32", "neg_s32", "stretch_s32", "partial_s32"])
def test_stage_entry_points_match_reference_golden(name, fm):
    """One reference function per launch: sampling, volume gather, projection gather, head, composite."""
    z, meta = load(name)
    sc = scene_of(meta)
    S, neg = meta["n_samples"], meta["neg_ray"]
    idx = z["st_rays"]                                    # 32 rays spread over the list; the wide arrays cover every 4th of them
    k, hv = idx.size, np.arange(0, idx.size, 4)
    assert np.array_equal(idx[hv], z["st_heavy"])
    fr = build_frame(fm, sc)
    rays = rays_of(sc)[torch.from_numpy(idx).to("cuda:0")]
    pts, zv, grid = fm.sample_points(fr, rays, S)
    # Geometry: the reference's bits.  Sample positions and grid coordinates are unfused IEEE operations in the reference's order, the
    # two small matrix products (world -> SMPL, K4 P4 [p, 1]) FMA chains over k as the reference's sgemm runs them (round 4), the
    # bilinear taps an FMA chain from the north-west tap as ATen's vectorised 2-D kernel sums them.
    assert np.array_equal(pts.cpu().numpy(), z["st_pts"]), "pts"
    assert np.array_equal(zv.cpu().numpy(), z["st_z"]), "z_vals"
    assert np.array_equal(grid.cpu().numpy().reshape(-1, 3), z["st_grid"]), "grid_coords"
    vf = fm.sample_volume(fr, grid)
    # (the trilinear taps are accumulated with FMAs here, with multiply-adds in ATen's scalar 3-D kernel: an ulp or two)
    e_vol = assert_close(vf.cpu().numpy().reshape(k, S, 128)[hv].reshape(-1, 128), z["st_vol_feat"], 2e-6, "volume features")
    feat, mask = fm.project_gather(fr, pts, neg_ray=neg)
    got_feat = feat.cpu().numpy().reshape(k, S, 3, 35)[hv]
    print(f"{name}: volume features max-abs {e_vol:.2e}; view features bit-equal on {float((got_feat == z['st_rgb_feat']).mean()):.4f} of the values, "
          f"max-abs {float(np.abs(got_feat - z['st_rgb_feat']).max()):.2e}")
    assert np.array_equal(got_feat, z["st_rgb_feat"]), "rgb_feat"
    assert np.array_equal(mask.cpu().numpy().reshape(k, S, 3), z["st_mask"])
    raw = fm.head_forward(fr.head_blob, vf, feat, mask)
    assert_close(raw.cpu().numpy().reshape(k, S, 4), z["st_raw"], TOL, "raw")
    comp = cpu(fm.composite(raw.reshape(k, S, 4), zv, mask.sum(-1).reshape(k, S), neg=neg))
    assert_close(comp["rgb_map"], z["rgb_map"][idx], TOL, "rgb_map")
    assert_close(comp["depth_map"], z["depth_map"][idx], TOL, "depth_map")
    assert_close(comp["weights"], z["weights"][idx], TOL, "weights")
    assert np.array_equal(comp["ray_mask"].astype(bool), z["st_ray_mask"])


def test_ray_order_changes_tiling_not_results(fm, syn):
    sc = syn.make_scene(H=40, W=48, seed=31, focal_mul=5.0, pose="random", aabb_half=(0.12, 0.16, 0.05), bias_std=0.1)
    fr = build_frame(fm, sc)
    rays = rays_of(sc)
    n = rays.shape[0]
    base = fm.render_fused(fr, rays, 16)
    order = torch.from_numpy(fm.patch_order(sc["mask_at_box"][0], 40, 48)).to("cuda:0")
    assert sorted(order.cpu().tolist()) == list(range(n))
    for o in (order, torch.randperm(n, device="cuda:0").int()):
        got = fm.render_fused(fr, rays, 16, ray_order=o)
        for k in base:
            assert torch.equal(torch.nan_to_num(got[k].float()), torch.nan_to_num(base[k].float())), k


CULL_CASES = [(False, False, False, None), (True, False, False, None), (False, True, False, None), (False, False, True, None), (True, True, True, None),
              (False, False, True, "mask"), (False, False, False, "in-loop")]


@pytest.mark.parametrize("neg,split_f16,lb,flip", CULL_CASES,
                         ids=[f"{n}-{sp}-{lb}" if fl is None else f"flip-{fl}" for n, sp, lb, fl in CULL_CASES])
def test_progressive_sample_culling_matches_restatement(neg, split_f16, lb, flip, fm, oracle, syn):
    """demo_render.py's occupancy / alpha culling against the oracle's restatement (itself pinned to outputs of that file,
    tests/golden/demo_*.npz): neg_ray (front test only -- the progressive integral never flips), both kernel forms and the
    sample-split launch geometry.

    flip: GPNERF_FLAG_OCC_CULL | GPNERF_FLAG_FLIP_SAMPLES, which the ABI takes and the oracle models (occ=, flip=True) although
    the progressive renderer never asks for it: composite step k keeps or culls SAMPLE S-1-k.  "mask": the keep bits computed
    before the launch into the workspace (occupancy_mask_kernel, Loop::CULLED -- a launch without per-sample outputs);
    "in-loop": the test inside the sample loop (no workspace)."""
    sc = syn.make_scene(H=24, W=24, seed=77, fill="full", pose="random", aabb_half=(0.2, 0.3, 0.12), bias_std=0.1,
                        vol_occupancy=0.35, neg_cams=neg)
    S = 48
    fr = build_frame(fm, sc)
    occ = fr.build_occupancy().cpu().numpy()
    occ_ref = oracle.build_occupancy(sc)
    assert_close(occ, occ_ref, 1e-4, "masks3d")
    assert 0.2 < (occ_ref > 0).mean() < 0.8
    if flip:
        ref = oracle.render(sc, S, stages=True, occ=occ_ref, flip=True)
        fwd = oracle.render(sc, S, stages=True, occ=occ_ref)
        # on the oracle's outputs: culling removes a good part of the samples that have density, not all of them, and the flipped
        # culled weights are far from the un-flipped ones on most rays that have any weight
        dense = oracle.render(sc, S, stages=True)["st_raw"][..., 3] > 0
        removed = (dense & (fwd["st_raw"][..., 3] == 0)).sum() / dense.sum()
        has = (ref["weights"].sum(1) > 0) | (fwd["weights"].sum(1) > 0)
        far = (np.abs(ref["weights"] - fwd["weights"]).max(1)[has] > 1e-2).mean()
        print(f"\n  oracle: culling removes {removed:.3f} of the samples with density; flipping moves the weights of {far:.3f} of the {has.sum()} rays that have any by > 1e-2")
        assert 0.2 < removed < 0.8 and has.sum() >= 64 and far >= 0.5
        rays = rays_of(sc)
        if flip == "mask":
            kw = dict(occ_cull=True, flip=True, neg_ray=False, load_balance=True, want=("z_vals", "rgb_in", "ray_mask"))
            plan = fm.render_plan(fr, rays, S, **kw)
            print(f"  plan: {plan}")
            assert plan.regions().get("mask"), str(plan)
            keys = ("rgb_map", "acc_map", "depth_map", "rgb_in_map")
        else:
            kw = dict(occ_cull=True, flip=True, neg_ray=False, load_balance=False, want=("weights", "raw", "z_vals", "rgb_in", "ray_mask"))
            keys = ("rgb_map", "acc_map", "depth_map", "weights", "rgb_in_map")
        got = cpu(fm.render_fused(fr, rays, S, **kw))
        for k in keys:
            print(f"  flip-{flip} {k}: max error against the oracle {assert_close(got[k], ref[k], TOL, k):.3g}")
        assert_close(got["z_vals"], ref["z_vals"], 1e-6, "z_vals")
        assert np.array_equal(got["ray_mask"].astype(bool), ref["ray_mask"].astype(bool))
        if "raw" in got:
            assert_close(got["raw"], ref["st_raw"], TOL, "raw")
        return
    got = cpu(fm.render_fused(fr, rays_of(sc), S, neg_ray=neg, occ_cull=True, split_f16=split_f16, load_balance=lb,
                              want=("weights", "raw", "z_vals", "rgb_in")))
    ref = oracle.render(sc, S, neg_ray=neg, stages=True, occ=occ_ref)
    for k in ("rgb_map", "acc_map", "depth_map", "weights", "rgb_in_map"):
        assert_close(got[k], ref[k], TOL, k)
    assert_close(got["z_vals"], ref["z_vals"], 1e-6, "z_vals")
    assert_close(got["raw"], ref["st_raw"], TOL, "raw")
    culled = (ref["st_raw"][..., 3] == 0).mean()
    dense = cpu(fm.render_fused(fr, rays_of(sc), S, neg_ray=neg))
    assert culled > 0.3 and np.abs(dense["acc_map"] - got["acc_map"]).max() > 1e-3, "the scene does not exercise culling"


def test_progressive_ray_selection_matches_restatement(fm, oracle, syn):
    """demo_render.py:166-247 on a non-512 frame against the oracle (pinned by tests/golden/demo_*.npz): index work, bit-exact."""
    H = W = 48
    sc = syn.make_scene(H=H, W=W, seed=78, focal_mul=6.0, pose="random", aabb_half=(0.2, 0.3, 0.12), vol_occupancy=0.3)
    fr = build_frame(fm, sc)
    occ_ref = oracle.build_occupancy(sc)
    K, P = sc["target_K"][0], sc["target_pose"][0]
    rays, mask = fm.select_rays(fr, K, P, H, W, sc["voxel_size"], sc["bounds"][0, 0], sc["Rh"][0], sc["Th"][0])
    ro, rd, near, far, mref = oracle.select_rays(occ_ref, sc["voxel_size"], sc["bounds"][0, 0], sc["Rh"][0], sc["Th"][0], P, K, H, W)
    rays, mask = rays.cpu().numpy(), mask.cpu().numpy()
    assert 50 < mref.sum() < H * W
    assert np.array_equal(mask, mref)
    assert np.array_equal(rays[:, 0:3], ro) and np.array_equal(rays[:, 3:6], rd), "rays"
    assert np.array_equal(rays[:, 6], near) and np.array_equal(rays[:, 7], far), "near / far"


@pytest.mark.parametrize("name", demo_case_names())
def test_progressive_ray_selection_matches_reference_fixtures(name, fm):
    """gpnerf_build_occupancy + gpnerf_select_pixels + gpnerf_make_rays_demo against values captured inside the reference's
    demo_render.py run: masks3d, mask_at_box, and the rays / near / far it handed to get_sampling_points -- bit-exact."""
    z, meta = load(name)
    sc = scene_of(meta)
    fr = build_frame(fm, sc)
    occ = fr.build_occupancy().cpu().numpy()
    assert_close(occ, z["masks3d"], demo_tolerances(name, TOL)[1], "masks3d")
    assert int((occ > 0.1).sum()) == int(z["n_mask_xyz"])
    rays, mask = fm.select_rays(fr, sc["target_K"][0], sc["target_pose"][0], 512, 512, sc["voxel_size"], sc["bounds"][0, 0],
                                sc["Rh"][0], sc["Th"][0], neg_ray=meta["neg_ray"], target_K_inv=z["target_K_inv"][0])
    rays, mask = rays.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal(mask, np.unpackbits(z["mask_at_box_bits"]).astype(bool)), "mask_at_box"
    assert np.array_equal(rays[:, 0:3], z["ray_o"]) and np.array_equal(rays[:, 3:6], z["ray_d"]), "rays"
    assert np.array_equal(rays[:, 6], z["near"]) and np.array_equal(rays[:, 7], z["far"]), "near / far"


@pytest.mark.parametrize("name", case_names())
def test_split_f16_mode_matches_reference_golden(name, fm):
    """GPNERF_FLAG_SPLIT_F16 (f16 hi/lo MFMA, fp32 accumulation) stays inside north_star's 1e-4 on every golden vector."""
    z, meta = load(name)
    sc = scene_of(meta)
    S = meta["n_samples"]
    fr = build_frame(fm, sc)
    got = cpu(fm.render_fused(fr, rays_of(sc), S, neg_ray=meta["neg_ray"], split_f16=True, want=("weights", "rgb_in", "raw", "ray_mask")))
    assert_close(got["rgb_map"], z["rgb_map"], TOL, "rgb_map")
    assert_close(got["depth_map"], z["depth_map"], TOL, "depth_map")
    assert_close(got["acc_map"], z["acc_map"], TOL, "acc_map")
    assert_close(got["rgb_in_map"], z["rgb_in_map"], TOL, "rgb_in_map")
    if "weights" in z:
        assert_close(got["weights"], z["weights"], TOL, "weights")
    if "st_raw" in z:
        assert_close(got["raw"][z["st_rays"]], z["st_raw"], TOL, "raw")


def test_random_scene_sweep_matches_oracle(fm, oracle, syn):
    """A seeded sweep over image sizes, sample counts, poses, focal lengths, neg_ray and both kernel forms
    (tools/parity_sweep.py runs the long version): errors stay two orders below north_star's bound, no ray-mask flips."""
    g = np.random.Generator(np.random.PCG64(77))
    worst = 0.0
    for case in range(10):
        H, W = int(g.choice([12, 16, 33])), int(g.choice([12, 20, 40]))
        S = int(g.choice([1, 3, 17, 64]))
        neg = bool(g.integers(0, 2))
        sc = syn.make_scene(H=H, W=W, seed=500 + case, fill=str(g.choice(["full", "survey"])), pose="random",
                            aabb_half=(0.1 + 0.1 * g.random(), 0.12 + 0.1 * g.random(), 0.04 + 0.04 * g.random()), bias_std=0.15,
                            sigma_bias=float(g.choice([0.0, 0.5])), neg_cams=neg, focal_mul=float(g.choice([0.6, 1.05, 2.0])))
        if sc["ray_o"].shape[1] == 0:
            continue
        fr = build_frame(fm, sc)
        ref = oracle.render(sc, S, neg_ray=neg)
        for split in (False, True):
            got = cpu(fm.render_fused(fr, rays_of(sc), S, neg_ray=neg, split_f16=split))
            for k in ("rgb_map", "depth_map", "acc_map", "rgb_in_map", "weights"):
                assert_close(got[k], ref[k], TOL, f"case {case} {k} split={split}")
                worst = max(worst, float(np.nanmax(np.abs(got[k].astype(np.float64) - ref[k])))) if got[k].size else worst
            assert np.array_equal(got["ray_mask"], ref["ray_mask"])
    assert worst < 2e-5, worst


@pytest.mark.parametrize("split_f16", [False, True])
def test_render_is_deterministic(split_f16, fm, syn):
    """No atomics, no order-dependent reductions on the per-ray path: two launches give identical bits (also with the
    sample-split launch geometry, whose segment merge runs in a fixed order)."""
    sc = syn.make_scene(H=48, W=48, seed=9, fill="full", pose="random", aabb_half=(0.12, 0.16, 0.05), bias_std=0.1)
    fr = build_frame(fm, sc)
    rays = rays_of(sc)
    for lb in (False, True):
        a = fm.render_fused(fr, rays, 32, split_f16=split_f16, load_balance=lb)
        b = fm.render_fused(fr, rays, 32, split_f16=split_f16, load_balance=lb)
        for k in a:
            assert torch.equal(a[k], b[k]), (k, lb)


@pytest.mark.parametrize("size,S,neg,split_f16,occupancy", [(24, 48, False, False, 0.35), (24, 48, True, True, 0.35), (40, 100, False, False, 0.2),
                                                            (272, 32, False, False, 0.1), (272, 24, False, True, 0.3)])
def test_culling_with_precomputed_keep_bits_equals_in_loop_test(size, S, neg, split_f16, occupancy, fm, oracle, syn):
    """Occupancy culling without per-sample outputs takes the form that computes every sample's keep bit before the launch, walks
    only the steps a tile keeps and (frames of more than one round of workgroups: the 272x272 cases) hands tiles out longest
    first.  Same bits as the form that tests inside the sample loop (chosen by asking for `weights`), and both match the oracle's
    restatement of demo_render.py:270-344."""
    sc = syn.make_scene(H=size, W=size, seed=91, fill="full", pose="random", aabb_half=(0.2, 0.3, 0.12), bias_std=0.1,
                        vol_occupancy=occupancy, neg_cams=neg)
    fr = build_frame(fm, sc)
    fr.build_occupancy()
    rays = rays_of(sc)
    order = torch.from_numpy(fm.patch_order(sc["mask_at_box"][0], size, size, 4, 8)).to("cuda:0")
    kw = dict(neg_ray=neg, occ_cull=True, split_f16=split_f16, load_balance=False, ray_order=order)
    in_loop = cpu(fm.render_fused(fr, rays, S, want=("weights",), **kw))
    masked = cpu(fm.render_fused(fr, rays, S, want=(), **kw))
    assert "weights" not in masked
    for k in masked:
        assert np.array_equal(masked[k].view(np.int32), in_loop[k].view(np.int32)), k
    again = cpu(fm.render_fused(fr, rays, S, want=(), **kw))
    for k in masked:
        assert np.array_equal(masked[k].view(np.int32), again[k].view(np.int32)), k
    pick = np.random.default_rng(5).choice(size * size, 256, replace=False)
    ref = oracle.render(sc, S, neg_ray=neg, rays=rays.cpu().numpy()[pick], occ=oracle.build_occupancy(sc))
    for k in ("rgb_map", "acc_map", "depth_map"):
        assert_close(masked[k][pick], ref[k], TOL, k)
    assert (in_loop["weights"].sum(-1) == 0).mean() > 0.05, "no ray of the scene is culled entirely"


@pytest.mark.parametrize("size,S,neg,kw", [(64, 32, False, {}), (96, 48, True, {}), (272, 24, False, {}), (272, 40, False, {"early_term": True, "term_eps": 1e-5}),
                                           (64, 32, False, {"occ_cull": True})])
def test_folded_coarse_levels_equal_the_layer_per_sample(size, S, neg, kw, fm, oracle, syn):
    """gpnerf_fold_volumes applies sigmahead.out_geometry_fc's columns of the two coarse levels to their voxels once per frame and
    the fp32 form interpolates that instead of running those columns per sample: Linear(sum w v) = sum w Linear(v), so the two
    agree to fp32 rounding (the big-frame tests of test_gpu_configs.py check the folded form against the oracle in its own right)."""
    sc = syn.make_scene(H=size, W=size, seed=3, fill="full", pose="random", aabb_half=(0.2, 0.3, 0.12), bias_std=0.1, neg_cams=neg,
                        **({"vol_occupancy": 0.35} if kw.get("occ_cull") else {}))
    fr = build_frame(fm, sc)
    rays = rays_of(sc)
    a = cpu(fm.render_fused(fr, rays, S, neg_ray=neg, want=("weights", "rgb_in"), fold=False, **kw))
    b = cpu(fm.render_fused(fr, rays, S, neg_ray=neg, want=("weights", "rgb_in"), fold=True, **kw))
    for k in ("rgb_map", "acc_map", "weights", "rgb_in_map"):
        assert_close(a[k], b[k], 5e-6, k)
    assert_close(a["depth_map"], b["depth_map"], 2e-5, "depth_map")
    # the default: the reference-order form (round 5), whatever the launch
    c = cpu(fm.render_fused(fr, rays, S, neg_ray=neg, want=("weights", "rgb_in"), **kw))
    for k in a:
        assert np.array_equal(np.nan_to_num(a[k]), np.nan_to_num(c[k])), k
    pick = np.random.default_rng(1).choice(rays.shape[0], 128, replace=False)
    if not kw:
        ref = oracle.render(sc, S, neg_ray=neg, rays=rays.cpu().numpy()[pick])
        for k in ("rgb_map", "acc_map", "depth_map"):
            assert_close(b[k][pick], ref[k], TOL, k)


def test_the_two_exits_of_the_reference_order_form_change_no_bit(fm, syn):
    """Where none of a step's 32 samples touches an active voxel the sigma feature layer is ELU(bias); where all 32 densities are
    exactly 0 (no source view sees the samples: masked_fill; ReLU) the colour branch cannot change a map.  The default form leaves
    both out, wave step by wave step, and reports how often (step_stats); every map is bit-identical to the launch that evaluates
    everything (GPNERF_FLAG_NO_EXITS) -- on a sparse person-shaped pyramid, on a frame whose source views miss part of the box, under
    early termination -- and a launch that returns `raw` (which needs every colour) agrees too."""
    cases = [dict(H=96, W=96, seed=81, fill="survey", pose="identity", body="capsules", sigma_bias=-1.0, bias_std=0.1, vol_scale=2.0),
             dict(H=64, W=64, seed=82, focal_mul=5.0, pose="random", aabb_half=(0.12, 0.16, 0.05), bias_std=0.1, sigma_bias=-0.5),
             dict(H=288, W=288, seed=83, fill="full", pose="identity", bias_std=0.1)]
    seen = [0, 0]
    for kw in cases:
        sc = syn.make_scene(**kw)
        fr = build_frame(fm, sc)
        rays = rays_of(sc)
        for extra in ({}, {"early_term": True, "term_eps": 1e-5}):
            want = ("weights", "z_vals", "rgb_in", "ray_mask", "step_stats")
            a = fm.render_fused(fr, rays, 48, want=want, **extra)
            b = fm.render_fused(fr, rays, 48, want=want, exits=False, **extra)
            st_a, st_b = a.pop("step_stats").cpu().numpy(), b.pop("step_stats").cpu().numpy()
            assert st_b[1] == 0 and st_b[2] == 0 and st_a[0] == st_b[0] > 0
            seen[0] += int(st_a[1]); seen[1] += int(st_a[2])
            for k in a:
                assert torch.equal(torch.nan_to_num(a[k].float()), torch.nan_to_num(b[k].float())), (kw.get("seed"), extra, k)
        r = fm.render_fused(fr, rays, 48, want=("raw", "weights"))
        assert torch.equal(r["rgb_map"], a["rgb_map"]) if not extra else True
        full = fm.render_fused(fr, rays, 48, want=("weights",))
        assert torch.equal(r["rgb_map"], full["rgb_map"]) and torch.equal(r["weights"], full["weights"])
    assert seen[0] > 0 and seen[1] > 0, f"the test scenes never took an exit: {seen}"


@pytest.mark.parametrize("form", ["reference-order", "folded", "split-f16", "split-f16-guarded"])
def test_deferred_colour_branch_is_the_plain_loop_bit_for_bit(form, fm, syn):
    """Every form's launches (the split-precision forms too since round 6: gpnerf_kernels.hip SPLIT_DEFERS -- round 5 held them back
    over one build's wrong colour passes, whose mechanism class is now measured and gated: an inline-asm operand conversion directly
    in front of the MFMA that reads it, tools/micro/asm_producer_hazards.hip, tests/test_abi.py) run the colour branch only for
    samples whose weight alpha * T is not zero, 32 at a time out of a per-wavefront queue (render_tile, DEFER).  Every map must be the bits of the launch that evaluates every colour
    (exits=False) -- ragged ray counts, fewer rays than a wavefront, 1 / 7 / 33 samples (queues that never fill, flushes of a few
    entries), a permuted ray order, small frames whose tiles are split over several wavefronts (load_balance), tile-level early
    termination without a workspace, both culling variants -- and step_stats counts the passes: none when every density is zero,
    one per step when none is."""
    sc = syn.make_scene(H=72, W=72, seed=91, fill="full", pose="random", aabb_half=(0.2, 0.3, 0.12), bias_std=0.1, sigma_bias=-0.3)
    fr = build_frame(fm, sc)
    rays_all = rays_of(sc)
    want = ("weights", "z_vals", "rgb_in", "ray_mask")
    g = torch.Generator().manual_seed(5)
    fkw = {"reference-order": {}, "folded": {"fold": True}, "split-f16": {"split_f16": True, "guard": False}, "split-f16-guarded": {"split_f16": True}}[form]
    render = lambda *a, **k: fm.render_fused(*a, **dict(fkw, **k))

    def same(a, b, tag):
        for k in a:
            assert torch.equal(torch.nan_to_num(a[k].float()), torch.nan_to_num(b[k].float())), (tag, k)

    fractions = []
    for n in (5, 31, 33, 1000, rays_all.shape[0] - 3):
        rays = rays_all[:n].contiguous()
        order = torch.randperm(n, generator=g).int().cuda()
        for S in (1, 7, 33, 64):
            # (neg_ray on this scene: the all-masked path -- no view sees a sample.  flip: the flipped order on the scene's density)
            for kw in ({}, {"ray_order": order}, {"load_balance": False}, {"early_term": True, "load_balance": False}, {"neg_ray": True}, {"flip": True}):
                if form == "split-f16-guarded" and kw.get("load_balance") is False:
                    continue                                   # (the guard keeps its state in the workspace)
                a = render(fr, rays, S, want=want + ("step_stats",), **kw)
                b = render(fr, rays, S, want=want, exits=False, **kw)
                st = a.pop("step_stats").cpu().numpy()
                same(a, b, (n, S, tuple(kw)))
                if (not kw or kw.get("flip")) and n >= 1000 and S == 64:
                    fractions.append(st[2] / st[0])
                    if kw.get("flip"):          # flipped, with density: another image than the forward order's
                        assert float((a["rgb_map"] - fwd["rgb_map"]).abs().max()) > 1e-2 and float(a["acc_map"].max()) > 0.1
                    else:
                        fwd = a
    assert len(fractions) == 4 and all(0.05 < f < 0.95 for f in fractions), fractions       # the scene does queue, and does skip, in both orders
    # progressive renderer's culling: keep bits computed before the launch (workspace) and tested sample by sample (none)
    sc3 = syn.make_scene(H=72, W=72, seed=93, fill="full", pose="random", aabb_half=(0.2, 0.3, 0.12), bias_std=0.1, vol_occupancy=0.3)
    fr3 = build_frame(fm, sc3)
    for kw in ({"occ_cull": True}, {"occ_cull": True, "load_balance": False}):
        if form == "split-f16-guarded" and kw.get("load_balance") is False:
            continue
        a = render(fr3, rays_of(sc3), 64, want=want, **kw)
        b = render(fr3, rays_of(sc3), 64, want=want, exits=False, **kw)
        same(a, b, tuple(kw))
    # exactly opaque rays (density bias + 60: T underflows to 0 behind four samples): the plain deferred loop stops gathering and
    # multiplying, keeps counting views for ray_mask and writing zero weights -- same bits, samples_done included
    sc4 = syn.make_scene(H=96, W=96, seed=94, fill="full", pose="random", aabb_half=(0.2, 0.3, 0.12), bias_std=0.1, sigma_bias=60.0)
    fr4 = build_frame(fm, sc4)
    for kw in ({}, {"load_balance": False}, {"neg_ray": True}, {"flip": True}):
        a = render(fr4, rays_of(sc4), 64, want=want + ("step_stats",), **kw)
        b = render(fr4, rays_of(sc4), 64, want=want, exits=False, **kw)
        st = a.pop("step_stats").cpu().numpy()
        same(a, b, ("opaque", tuple(kw)))
        if not kw.get("neg_ray"):       # (with the front test inverted no view sees a sample: no density at all)
            assert st[1] > 0.2 * st[0], st                     # many steps sit behind the surface (a small frame splits its tiles: each segment starts at T = 1)
        a = render(fr4, rays_of(sc4), 64, want=("samples_done", "ray_mask"), **kw)
        b = render(fr4, rays_of(sc4), 64, want=("samples_done", "ray_mask"), exits=False, **kw)
        same(a, b, ("opaque samples_done", tuple(kw)))
    # no density anywhere: not one colour pass; density everywhere: one pass per step
    # (3 samples for the second: behind an opaque sample T = 1e-10, 1e-20, ... underflows to zero weights after four)
    for bias, S, expect in ((-60.0, 64, "none"), (60.0, 3, "all")):
        sc2 = syn.make_scene(H=64, W=64, seed=92, fill="full", pose="identity", sigma_bias=bias)
        fr2 = build_frame(fm, sc2)
        a = render(fr2, rays_of(sc2), S, want=want + ("step_stats",))
        b = render(fr2, rays_of(sc2), S, want=want, exits=False)
        st = a.pop("step_stats").cpu().numpy()
        same(a, b, expect)
        assert (st[2] == st[0]) if expect == "none" else (st[2] == 0), (expect, st)


@pytest.mark.parametrize("form", ["reference-order", "folded"])
def test_frame_level_deferral_is_the_wavefront_level_one_bit_for_bit(form, fm, syn):
    """Frames of more than one round of wavefronts list the samples whose weight is not zero and evaluate the list in a second,
    balanced launch (colour_units_kernel; colour_accumulate_kernel adds a ray's terms in sample order) where the workspace has room
    for the list; with less workspace every wavefront runs its own colour passes.  Same arithmetic on the same operands in the same
    order: every map must be the same bits, on every launch shape that lists -- whole rounds on the tile queue, whole rounds plus a
    remainder launch, one launch of whole tiles and eight-samples-per-step units (a ZJU-sized frame), the chained segments of early
    termination -- and step_stats must count exactly ceil(non-zero weights / 32) colour evaluations (a packed list) where the
    wavefront-level passes count at least as many."""
    fkw = {"reference-order": {}, "folded": {"fold": True}}[form]
    want = ("weights", "z_vals", "rgb_in", "ray_mask")
    g = torch.Generator().manual_seed(9)
    small = 48 << 20           # room for the tile queue and the chained form's lists, not for a frame's entry list

    def same(a, b, tag):
        for k in a:
            assert torch.equal(torch.nan_to_num(a[k].float()), torch.nan_to_num(b[k].float())), (tag, k)

    listed, listed_flipped = 0, 0
    # (the last two: nearly every weight non-zero -- the list at its worst-case capacity, every visit's padded unit on top)
    for size, S, bias in ((362, 64, -0.3), (260, 64, -0.3), (370, 33, -0.3), (300, 128, 1.0), (260, 8, 3.0), (362, 8, 3.0)):
        sc = syn.make_scene(H=size, W=size, seed=100 + size, fill="full", pose="random", aabb_half=(0.2, 0.3, 0.12), bias_std=0.1, sigma_bias=bias)
        fr = build_frame(fm, sc)
        rays_all = rays_of(sc)
        for n in (rays_all.shape[0], rays_all.shape[0] - 37):
            rays = rays_all[:n].contiguous()
            order = torch.randperm(n, generator=g).int().cuda()
            # (neg_ray on these scenes: the all-masked path, nothing to list.  flip: the flipped order on the scene's own density --
            #  the list's entries recompute their sample point from S-1-k)
            for kw in ({}, {"ray_order": order}, {"neg_ray": True}, {"flip": True}, {"early_term": True, "term_eps": 1e-5}):
                if (kw.get("neg_ray") or kw.get("flip")) and n != rays_all.shape[0]:
                    continue
                if S == 128 and not kw.get("early_term"):
                    continue        # (1.4 rounds: with the small workspace this frame splits its tiles' samples -- another association of T)
                pa = fm.render_plan(fr, rays, S, want=want + ("step_stats",), **dict(fkw, **kw))
                pb = fm.render_plan(fr, rays, S, want=want + ("step_stats",), workspace_cap=small, **dict(fkw, **kw))
                for pl in (pa, pb):
                    assert ("list" in pl.regions()) == (pl.triple()[1] in ("LIST", "UNIFIED")) and pl.triple()[2] == ("FOLD" if fkw else "REF"), str(pl)
                assert "list" in pa.regions() or "list" not in pb.regions()         # less workspace never lists where more does not
                a = fm.render_fused(fr, rays, S, want=want + ("step_stats",), **dict(fkw, **kw))
                b = fm.render_fused(fr, rays, S, want=want + ("step_stats",), workspace_cap=small, **dict(fkw, **kw))
                sa, sb = a.pop("step_stats").cpu().numpy().astype(np.int64), b.pop("step_stats").cpu().numpy().astype(np.int64)
                same(a, b, (size, S, n, tuple(kw)))
                if n == rays_all.shape[0]:          # GPNERF_FLAG_SHARED_DEVICE: the list always goes to the second kernel -- the same bits
                    c = fm.render_fused(fr, rays, S, want=want, shared_device=True, **dict(fkw, **kw))
                    same(c, b, (size, S, n, tuple(kw), "shared device"))
                # (steps and opaque tails are the launch's; the units of several samples per step take the level-by-level exit of the
                #  sigma feature layer only when they list: never fewer levels left out)
                assert sa[0] == sb[0] and sa[3] == sb[3] and sa[1] >= sb[1] and sa[4] >= sb[4], (sa, sb)
                assert sa[5] <= sb[5] and sa[2] == sa[0] - sa[5], (sa, sb)
                units = (int((a["weights"] != 0).sum()) + 31) // 32
                if not kw:
                    fwd = a
                if kw.get("flip"):      # flipped, with density: as many samples to colour as a tenth of the forward order's at least, another image
                    assert units * 10 >= (int((fwd["weights"] != 0).sum()) + 31) // 32 > 0 and float((a["rgb_map"] - fwd["rgb_map"]).abs().max()) > 1e-2
                if "list" not in pa.regions():      # no list, no packed evaluation: the launches counted below are the ones planned to list
                    assert sa[5] == sb[5], (size, S, n, tuple(kw), str(pa), sa, sb)
                if n == rays_all.shape[0]:
                    pc = fm.render_plan(fr, rays, S, want=want, shared_device=True, **dict(fkw, **kw))
                    assert pc.triple()[1] != "UNIFIED" and ("list" in pc.regions()) == ("list" in pa.regions()), str(pc)
                if sa[5] < sb[5]:
                    listed += 1
                    listed_flipped += bool(kw.get("flip"))
                    assert "list" in pa.regions() and "list" not in pb.regions() and pa.triple()[0] != "STATIC", (size, S, n, tuple(kw), str(pa), str(pb))
                    # a packed list: exactly `units` evaluations where a second kernel walks it; where the launch's own wavefronts do
                    # (plain launches on the tile queue, the one-launch ZJU-sized shape) every tile pads its last unit
                    assert units <= sa[5], (size, S, n, tuple(kw), sa, units)
                    if kw.get("early_term"):
                        assert sa[5] == units, (size, S, n, tuple(kw), sa, units)
                else:           # a launch shape that does not list (a frame between one and two rounds splits its tiles' samples instead)
                    assert sa[5] == sb[5], (size, S, n, tuple(kw), sa, sb)
        if S != 128:
            c = fm.render_fused(fr, rays_all, S, want=want, exits=False, **fkw)
            a = fm.render_fused(fr, rays_all, S, want=want, **fkw)
            same(a, c, (size, S, "every layer of every sample"))
    # the launches did take the frame-level path: a packed list needs fewer evaluations than per-wavefront passes (frames of two
    # round without a remainder launch evaluate the list themselves and pad what a tile leaves to a whole unit: the
    # per-wavefront count, 362 x 362 here).  12 in the forward order: the eight early-terminated launches of the first four frames
    # and the four launches of 370 x 370 x 33, whose list a second kernel walks; and one more in the flipped order at least, the
    # flipped 370 x 370 x 33 launch (QUEUE_REMAINDER / LIST): 13.
    print(f"\n  launches that needed fewer colour evaluations with the frame's list: {listed}, {listed_flipped} of them flipped")
    assert listed >= 13 and listed_flipped >= 1, (listed, listed_flipped)


def test_reserved_cus_render_the_same_frame(fm, syn):
    """GPNERF_FLAG_RESERVE_CUS plans the launch for fewer compute units (the pipelined loop's experiment, profiles/r05/d_pipeline.txt).
    A ray's result is a function of the ray alone, so the maps are the ones a smaller chip gives: bit-identical whenever the launch
    geometry stays one wavefront per tile (always under early termination), and within the documented ~1e-7 re-association of the
    transmittance product when the smaller chip makes the launch split a tile's samples over several wavefronts
    (include/gpnerf_hip.h, `workspace`)."""
    sc = syn.make_scene(H=288, W=288, seed=71, fill="full", pose="random", aabb_half=(0.2, 0.3, 0.12), bias_std=0.1, sigma_bias=1.0)
    fr = build_frame(fm, sc)
    rays = rays_of(sc)
    for kw in ({}, {"early_term": True, "term_eps": 1e-5}):
        base = fm.render_fused(fr, rays, 48, want=("weights", "rgb_in"), **kw)
        full = fm.render_plan(fr, rays, 48, want=("weights", "rgb_in"), **kw)
        for reserve in (8, 64, 200, 255):
            plan = fm.render_plan(fr, rays, 48, want=("weights", "rgb_in"), reserve_cus=reserve, **kw)
            # planned for the smaller chip (whole XCD rounds of 8, at least 8 stay): the plan is the one that chip itself gets
            assert plan.n_cus == max(full.n_cus - (reserve & ~7), min(full.n_cus, 8))
            assert plan.triple()[0] == "STATIC" or plan.grid <= plan.n_cus, str(plan)
            small_chip = fm.render_plan(fr, rays, 48, want=("weights", "rgb_in"), n_cus=plan.n_cus, **kw)
            assert (plan.triple(), plan.waves, plan.split, plan.grid, plan.regions()) == (small_chip.triple(), small_chip.waves, small_chip.split,
                                                                                         small_chip.grid, small_chip.regions())
            if kw:          # one wavefront per whole tile: why the bits below are the same
                assert plan.split == 1 and full.split == 1, (str(full), str(plan))
            got = fm.render_fused(fr, rays, 48, want=("weights", "rgb_in"), reserve_cus=reserve, **kw)
            for k in base:
                a, b = torch.nan_to_num(base[k]), torch.nan_to_num(got[k])
                if kw:
                    assert torch.equal(a, b), (kw, reserve, k)
                else:
                    assert float((a - b).abs().max()) <= 2e-6, (reserve, k)
    base = fm.render_fused(fr, rays, 48, want=("weights", "rgb_in"))
    p0, p7 = (fm.render_plan(fr, rays, 48, want=("weights", "rgb_in"), reserve_cus=r) for r in (0, 7))
    assert str(p0) == str(p7)
    same = fm.render_fused(fr, rays, 48, want=("weights", "rgb_in"), reserve_cus=7)          # rounded down to whole XCD rounds: nothing reserved
    assert all(torch.equal(torch.nan_to_num(base[k]), torch.nan_to_num(same[k])) for k in base)



def test_a_frame_that_gets_new_volumes_drops_what_it_derived_from_the_old_ones(fm, syn):
    """Frame._set_volumes on a used Frame: the folded coarse levels and the occupancy volume belong to the old levels;
    kept, the next dense launch would interpolate the old tables with the new levels' dimensions."""
    a = syn.make_scene(H=16, W=16, seed=61, fill="full", pose="random", aabb_half=(0.12, 0.16, 0.05), bias_std=0.1)
    b = syn.make_scene(H=16, W=16, seed=62, fill="full", pose="random", aabb_half=(0.12, 0.16, 0.05), bias_std=0.1)
    fr = build_frame(fm, a)
    rays = rays_of(a)
    first = fm.render_fused(fr, rays, 32, fold="keep")            # folds level 2 and 3 of scene a
    fr.build_occupancy()
    assert fr._folded_valid and fr.c.occ
    fr._set_volumes(fr.c, [to_dev(v * 0.5) for v in b["volumes"]], fr._keep)
    assert not fr._folded_valid and fr.vols_folded is None and fr.occ is None and not fr.c.occ
    got = fm.render_fused(fr, rays, 32, fold="keep")
    fresh_scene = dict(a, volumes=[v * 0.5 for v in b["volumes"]])
    want = fm.render_fused(build_frame(fm, fresh_scene), rays, 32, fold="keep")
    assert torch.equal(got["rgb_map"], want["rgb_map"]) and torch.equal(got["depth_map"], want["depth_map"])
    assert not torch.equal(got["rgb_map"], first["rgb_map"])


@pytest.mark.parametrize("H,W,pw,ph,fill", [(512, 512, 32, 8, 0.3), (512, 512, 8, 4, 0.28), (64, 48, 8, 4, 0.5), (37, 45, 32, 8, 0.7),
                                            (128, 96, 4, 8, 1.0), (40, 40, 32, 8, 0.0), (70, 200, 24, 5, 0.6), (1024, 1024, 32, 8, 0.2)])
def test_patch_order_kernels_equal_the_host_function(H, W, pw, ph, fill):
    """gpnerf_patch_order (three launches, no host round trip) gives frame.patch_order()'s permutation for any mask -- ragged bands
    and patches, patch widths that do not divide the 64-pixel window, empty and full masks -- and the identity when the mask does not
    keep exactly the caller's n pixels."""
    fm = importlib.import_module("gp-nerf_amd.frame")
    g = np.random.default_rng(H * W + pw)
    mask = g.random(H * W) < fill
    if fill == 0.3:                       # a body-shaped blob rather than noise: whole empty rows and patches
        yy, xx = np.mgrid[0:H, 0:W]
        mask = (((yy - H / 2) / (0.4 * H)) ** 2 + ((xx - W / 2) / (0.2 * W)) ** 2 < 1).reshape(-1)
    n = int(mask.sum())
    want = fm.patch_order(mask, H, W, patch_w=pw, patch_h=ph)
    md = torch.from_numpy(mask).to("cuda:0")
    got = fm.patch_order_rays(md, H, W, n, patch_w=pw, patch_h=ph)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(fm.patch_order_rays(md.to(torch.uint8), H, W, n, patch_w=pw, patch_h=ph).cpu().numpy(), want)
    if n > 3:
        wrong = fm.patch_order_rays(md, H, W, n - 3, patch_w=pw, patch_h=ph)
        assert np.array_equal(wrong.cpu().numpy(), np.arange(n - 3))
