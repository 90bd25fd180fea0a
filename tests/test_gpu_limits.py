"""GPU: the gathers and the per-sample output rows at the addressing limits include/gpnerf_hip.h promises (every tensor below 2^32
bytes, every x-row below 2^24 bytes, every row count below 2^24).  tests/test_abi.py checks that frames beyond them are refused and
that their neighbours inside are accepted; here a kernel runs on each extreme shape: tap offsets with bit 31 set, __umul24 operands
next to 2^24, `raw` rows beyond 2^31 bytes -- against a plain-torch float64 reference (tests/limit_cases.py), one large tensor swapped
into an ordinary small frame at a time.  Every case prints its tensor's bytes, the largest tap offset the reference reached, the
share of points with a tap beyond 2^31 and the measured errors."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import limit_cases as LC
from limit_cases import CH, DEV, FOLDED_BYTES, HALF, INDEX_SLACK, LIM24, LIM_BYTES, PIXEL_BYTES, TOL_FEAT, TOL_RAW, VOXEL_BYTES

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def fm():
    return importlib.import_module("gp-nerf_amd.frame")


def need(nbytes):
    if LC.total_memory() < nbytes:
        pytest.skip(f"the device has {LC.total_memory() >> 30} GiB in all, the case needs {nbytes >> 30}")


def bits(t):
    return t.contiguous().view(torch.int32)


def max_err(got, ref, keep):
    """max |got - ref| over the kept rows (or entries), per trailing column"""
    d = (got.double() - ref).abs()
    d = torch.where(keep.to(d.device).reshape(keep.shape + (1,) * (d.dim() - keep.dim())), d, torch.zeros_like(d))
    return d.reshape(-1, d.shape[-1]).amax(0)


def fold_matrix(fm, syn, level, sc):
    """The 64 x 32 map gpnerf_fold_volumes applies to a voxel of `level`, in its own output layout: the folded values of 32 one-hot
    voxels (1 x w + 0 is exact).  Checked here to be sigmahead.out_geometry_fc.0's 32 columns of that level, x log2(e) (the folded
    form's scaled domain), its 64 rows in the layout's order -- so the product below IS the layer's."""
    fr, _, _ = LC.small_frame(fm, syn)
    hot = torch.zeros((2, 4, 4, CH), device=DEV)
    hot.view(32, CH)[torch.arange(32), torch.arange(32)] = 1.0
    LC.swap_level(fr, level, hot)
    M = fr.fold_volumes()[level].reshape(32, 2 * CH).t().double().cpu()                 # [64 outputs (layout order), 32 channels]
    Wl = torch.from_numpy(sc["head"]["sigmahead.out_geometry_fc.0.weight"][:, CH * level:CH * (level + 1)].astype(np.float64)) * LOG2E
    dist = (M[:, None, :] - Wl[None, :, :]).abs().amax(2)                                # [layout row, layer row]
    row = dist.argmin(1)
    assert sorted(row.tolist()) == list(range(2 * CH)) and float(dist.min(1).values.max()) <= 1e-6 * float(Wl.abs().max()) + 1e-7
    return M


# ---- volume levels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,kind", [(0, "rows"), (0, "row_bytes"), (2, "rows"), (2, "row_bytes")])
def test_a_volume_level_at_the_limit(level, kind, fm, syn):
    """sample_volume, query_points and render_fused (reference-order, split-f16 and, on level 2, folded) with one level at the
    extreme shape: level 0 [4095, 4097, 2] (x-row index up to 2^24 - 2, 2^32 - 256 bytes) and [16, 16, 131071] (x-rows of 2^24 - 128
    bytes); level 2, whose folded twin has 256 bytes per voxel, [2048, 4095, 2] (folded: 2^32 - 2^20 bytes) and [16, 16, 65535]
    (folded x-rows of 2^24 - 256 bytes).  gpnerf_fold_volumes' output on those two is checked against the float64 product of the
    layer's columns with sampled voxels; the bound there is fp32 summation's a-priori 32 u sum|w||v|, u = 2^-24."""
    cell = FOLDED_BYTES if level >= 2 else VOXEL_BYTES
    D, H, W = LC.level_shape(kind, cell)
    nbytes, widest = D * H * W * VOXEL_BYTES, D * H * W * cell
    if kind == "rows":
        assert (D, H, W) == ((4095, 4097, 2) if level == 0 else (2048, 4095, 2))
        assert (D * H == LIM24 - 1 and widest == LIM_BYTES - 256) if level == 0 else widest == LIM_BYTES - (1 << 20)
    else:
        assert W * cell == LIM24 - cell and (D, H, W) == (16, 16, 131071 if level == 0 else 65535)
        assert widest == LIM_BYTES - 256 * cell
    need(nbytes + (widest if level >= 2 else 0) + (2 << 30))
    fr, blob, sc = LC.small_frame(fm, syn)
    vol = LC.big_rand((D, H, W, CH), seed=100 + level)
    LC.swap_level(fr, level, vol)
    pts = LC.make_points((LC.lattice_bits(W), LC.lattice_bits(H), LC.lattice_bits(D)), outer=2, seed=level)
    g = pts - 1.0
    refs = [LC.ref_volume(fr.vols[l], g) for l in range(4)]
    vol_ref = torch.cat([r[0] for r in refs], 1)
    taps, slack = refs[level][1], sum(r[2] for r in refs)
    ok = slack <= INDEX_SLACK
    top, share, tail = LC.reach(taps, cell, widest)
    print(f"level {level} {kind}: [{D}, {H}, {W}] {nbytes} bytes ({widest} in its widest form), largest tap offset {top}, "
          f"{100 * share:.1f} % of {len(pts)} points beyond 2^31, {int(ok.sum())} compared")
    assert share >= 0.5 and tail and bool(ok[:66].all()) and float(ok.double().mean()) >= 0.9
    assert float(vol.abs().max()) <= 1.0

    got = fm.sample_volume(fr, g.to(DEV))
    e_vol = float(max_err(got, vol_ref, ok).max())
    feat_ref, mask_ref, _, _, vslack = LC.ref_views(fr.imgs, fr.featmaps, LC.view_scales(fr), pts)
    raw_ref = fm.head_forward(blob, vol_ref.float(), feat_ref.float(), mask_ref.to(DEV)).double()
    ok_raw = ok & (vslack <= INDEX_SLACK).all(1)
    errs = {"query_points": float(max_err(fm.query_points(fr, pts.to(DEV))["raw"], raw_ref, ok_raw).max())}
    rays = LC.point_rays(pts)
    forms = {"reference-order": {}, "split-f16": {"split_f16": True}}
    if level >= 2:
        forms["folded"] = {"fold": True}
    raws = {}
    for name, kw in forms.items():
        raws[name] = fm.render_fused(fr, rays, 1, want=("raw",), **kw)["raw"].reshape(-1, 4)
        assert bool(torch.isfinite(raws[name]).all()), name
        errs[name] = float(max_err(raws[name], raw_ref, ok_raw).max())
    print(f"level {level} {kind}: sample_volume max-abs {e_vol:.2e} (bound {TOL_FEAT:.0e}); raw max-abs " +
          ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {TOL_RAW:.0e})")
    assert e_vol <= TOL_FEAT
    for k, v in errs.items():
        assert v <= TOL_RAW, (k, v)
    if level >= 2:
        # the folded launch really read the folded level (the reference-order form's bits would be the default's) ...
        assert fr.c.vol_folded[level] and not torch.equal(bits(raws["folded"]), bits(raws["reference-order"]))
        # ... and gpnerf_fold_volumes wrote it right, up to the last voxel
        folded = fr.vols_folded[level]
        assert folded.numel() * 4 == widest
        M = fold_matrix(fm, syn, level, sc).to(DEV)
        n = D * H * W
        idx = torch.cat([torch.tensor([0, n - 1]), torch.randint(0, n, (4096,), generator=torch.Generator().manual_seed(3))]).to(DEV)
        v = vol.view(-1, CH)[idx].double()
        want = v @ M.t()
        bound = 32 * 2.0 ** -24 * (v.abs() @ M.abs().t())
        diff = (folded.view(-1, 2 * CH)[idx].double() - want).abs()
        print(f"level {level} {kind}: folded voxels max-abs {float(diff.max()):.2e}, largest error / bound {float((diff / bound).max()):.3f}")
        assert bool((diff <= bound).all())
    del fr, vol, got, raws
    LC.release()


# ---- feature maps and images ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,kind", [("featmaps", "row_bytes"), ("featmaps", "rows"), ("images", "row_bytes")])
def test_the_view_maps_at_the_limit(what, kind, fm, syn):
    """project_gather, query_points and render_fused's rgb_in (deferred-colour and split-f16 forms) with every view's feature map at
    [256, 131071] (rows of 2^24 - 128 bytes) and [16777215, 2] (row index up to 2^24 - 2), and every view's image at [256, 1048575]
    (rows of 2^24 - 16 bytes).  The projector's clamp to +-1e6 keeps the image's last 48 575 columns unreachable (the reference
    clamps alike, and a clamped column is not on the lattice float32 resolves exactly): there the farthest compared tap is column
    983 039 of the last row, 2^20 bytes from the view's end, where the other cases reach the last 256 bytes.
    rgb_in_map of a one-sample ray is weight x rgb_in (one fma), so it is held to the gathers' bound against weight x reference."""
    cell = VOXEL_BYTES if what == "featmaps" else PIXEL_BYTES
    h, w = LC.map_shape(kind, cell)
    nbytes = h * w * cell
    if kind == "rows":
        assert h == LIM24 - 1 and w == 2 and nbytes == LIM_BYTES - 256
    else:
        assert w * cell == LIM24 - cell and h == 256 and w == (131071 if what == "featmaps" else 1048575)
    need(3 * nbytes + (2 << 30))
    fr, blob, sc = LC.small_frame(fm, syn)
    big = LC.big_rand((3, h, w, cell // 4), seed=200 + h % 7)
    if what == "featmaps":
        LC.swap_featmaps(fr, big)
    else:
        LC.swap_images(fr, big)
    bx, by = LC.lattice_bits(fr.c.img_w, fr.c.feat_w), LC.lattice_bits(fr.c.img_h, fr.c.feat_h)
    pts = LC.make_points((bx, by, 12), outer=1, seed=h % 11)
    if what == "images":        # the last exact column under the clamp, in the last row, for the views with s_x = (W - 1) / 2 and W - 1
        assert bx == 4
        pts = torch.cat([pts, torch.tensor([[30.0 / 16, 2.0, 0.5], [15.0 / 16, 0.5, 0.5]])])
    feat_ref, mask_ref, itaps, ftaps, slack = LC.ref_views(fr.imgs, fr.featmaps, LC.view_scales(fr), pts)
    ok = slack <= INDEX_SLACK                                                             # [P, V]
    top, share, tail = LC.reach(ftaps if what == "featmaps" else itaps, cell, nbytes, tail=256 if what == "featmaps" else 1 << 20)
    print(f"{what} {kind}: [3, {h}, {w}] {nbytes} bytes per view, largest tap offset {top}, {100 * share:.1f} % of {len(pts)} points "
          f"beyond 2^31, {int(ok.sum())} of {ok.numel()} (point, view) pairs compared, {int(mask_ref.sum())} in view")
    # (compared pairs: all but the edge points -- and, on the wide image, the columns the clamp moves off the lattice)
    assert share >= 0.5 and tail and float(ok.double().mean()) >= 0.75 and 0.2 <= float(mask_ref.mean()) <= 0.8
    vmax_i, vmax_f = max(1.0, float(fr.imgs.abs().max())), max(1.0, float(fr.featmaps.abs().max()))
    assert float(big.abs().max()) <= 1.0
    tol = torch.tensor([TOL_FEAT * vmax_i] * 3 + [TOL_FEAT * vmax_f] * CH, dtype=torch.float64, device=DEV)

    feat, mask = fm.project_gather(fr, pts.to(DEV))
    e_feat = max_err(feat, feat_ref, ok)
    assert torch.equal(mask.cpu(), mask_ref), f"{int((mask.cpu() != mask_ref).sum())} masks differ"
    g = pts - 1.0
    vol_ref = torch.cat([LC.ref_volume(fr.vols[l], g)[0] for l in range(4)], 1)
    raw_ref = fm.head_forward(blob, vol_ref.float(), feat_ref.float(), mask_ref.to(DEV)).double()
    ok_pt = ok.all(1)
    e_query = float(max_err(fm.query_points(fr, pts.to(DEV))["raw"], raw_ref, ok_pt).max())
    rays = LC.point_rays(pts)
    e_in, e_rgb, lit = {}, {}, {}
    for name, kw in {"reference-order": {}, "split-f16": {"split_f16": True}}.items():
        r = fm.render_fused(fr, rays, 1, want=("rgb_in", "weights"), **kw)
        w0 = r["weights"][:, 0].double()
        lit[name] = float((w0 > 0).double().mean())
        e_in[name] = max_err(r["rgb_in_map"].reshape(-1, 3, 3), w0[:, None, None] * feat_ref[:, :, :3], ok)
        e_rgb[name] = float(max_err(r["rgb_map"], w0[:, None] * raw_ref[:, :3], ok_pt).max())
    print(f"{what} {kind}: project_gather max-abs rgb {float(e_feat[:3].max()):.2e} (bound {TOL_FEAT * vmax_i:.1e}), features "
          f"{float(e_feat[3:].max()):.2e} (bound {TOL_FEAT * vmax_f:.1e}); query_points raw {e_query:.2e} (bound {TOL_RAW:.0e}); rgb_in " +
          ", ".join(f"{k} {float(v.max()):.2e}" for k, v in e_in.items()) + "; rgb_map " + ", ".join(f"{k} {v:.2e}" for k, v in e_rgb.items()) +
          f"; weight > 0 on {100 * lit['reference-order']:.0f} % of the points")
    assert bool((e_feat <= tol).all())
    assert e_query <= TOL_RAW
    for name in e_in:
        assert lit[name] >= 0.125, "too few points with a weight: rgb_in would check nothing"
        assert bool((e_in[name] <= tol[:3]).all()) and e_rgb[name] <= TOL_RAW, name
    del fr, big, feat
    LC.release()


# ---- occupancy -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rows", "row_bytes"])
def test_the_occupancy_volume_at_the_limit(kind, fm, syn):
    """sample_occupancy's 24 x 24-bit product on a level-0-sized occupancy of [4095, 4097, 2] and [16, 16, 131071]: the keep / cull
    decisions of query_points(occ_cull=True) and render_fused(occ_cull=True) over a sparse NON-NEGATIVE occupancy, where a point is
    kept exactly when one of its taps with weight holds a positive value, whatever the summation order (the argument of
    test_gpu_mesh.py); compared where float32 and float64 agree on which taps carry weight (under the cull the grid coordinates divide
    by the literal 0.005, so the points are not on the exact lattice).  And gpnerf_build_occupancy on the large level 0 against
    float64 channel sums at sampled voxels, the last included, within fp32 summation's a-priori 127 u sum|x|."""
    D, H, W = LC.level_shape(kind, VOXEL_BYTES)
    n = D * H * W
    assert (D * H == LIM24 - 1) if kind == "rows" else (W == 131071)
    need(n * (VOXEL_BYTES + 3 * LC.OCC_BYTES) + (2 << 30))
    fr, blob, sc = LC.small_frame(fm, syn)
    vol = LC.big_rand((D, H, W, CH), seed=300)
    LC.swap_level(fr, 0, vol)
    # gpnerf_build_occupancy: F.interpolate(mode="nearest") of every level to level 0's size, channels summed
    occ = fr.build_occupancy()
    idx = torch.cat([torch.tensor([0, n - 1]), torch.randint(0, n, (4096,), generator=torch.Generator().manual_seed(5))])
    d, hh, ww = idx // (H * W), (idx // W) % H, idx % W
    total, mag = torch.zeros(len(idx), dtype=torch.float64, device=DEV), torch.zeros(len(idx), dtype=torch.float64, device=DEV)
    for l in range(4):
        Dl, Hl, Wl = fr.vols[l].shape[:3]
        lin = ((d * Dl // D).clamp(max=Dl - 1) * Hl + (hh * Hl // H).clamp(max=Hl - 1)) * Wl + (ww * Wl // W).clamp(max=Wl - 1)
        x = fr.vols[l].view(-1, CH)[lin.to(DEV)].double()
        total += x.sum(1)
        mag += x.abs().sum(1)
    diff = (occ.view(-1)[idx.to(DEV)].double() - total).abs()
    bound = 127 * 2.0 ** -24 * mag
    print(f"occupancy {kind}: built [{D}, {H}, {W}] {n * 4} bytes from a level 0 of {n * VOXEL_BYTES}; channel sums max-abs "
          f"{float(diff.max()):.2e}, largest error / bound {float((diff / bound).max()):.3f}")
    assert bool((diff <= bound).all())
    # the cull over an occupancy of the test's own: 8 % of the voxels positive
    del occ
    own = torch.rand((D, H, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    own = torch.where(own < 0.08, own + 0.5, torch.zeros_like(own))
    fr.occ = own
    fr.c.occ = own.data_ptr()
    lat = LC.make_points((LC.lattice_bits(W), LC.lattice_bits(H), LC.lattice_bits(D)), outer=2, seed=9)
    c = torch.tensor(0.005, dtype=torch.float32)
    pts = lat * c                                           # p with p / 0.005 next to the lattice value (exactly 0 and 2 at the ends)
    g = (((pts - 0.0) / c) / 2.0) * 2.0 - 1.0               # grid_coords under the cull, float32: out_sh = 2, bounds_min = 0
    assert g.dtype == torch.float32 and float(g[0].abs().max()) == 1.0 and bool((g[1] == 1.0).all())
    (jx, wx, _), (jy, wy, _), (jz, wz, _) = LC.axis_taps(g[:, 0], W), LC.axis_taps(g[:, 1], H), LC.axis_taps(g[:, 2], D)
    same = LC.same_taps(g[:, 0], W) & LC.same_taps(g[:, 1], H) & LC.same_taps(g[:, 2], D)
    keep = torch.zeros(len(pts), dtype=torch.bool)
    taps = []
    flat = own.view(-1)
    for a in range(2):
        for b in range(2):
            for e in range(2):
                wgt = wz[:, a] * wy[:, b] * wx[:, e]
                lin = (jz[:, a] * H + jy[:, b]) * W + jx[:, e]
                keep |= (wgt > 0) & (flat[lin.to(DEV)].cpu() > 0)
                taps.append(torch.where(wgt > 0, lin, torch.full_like(lin, -1)))
    top, share, tail = LC.reach(torch.stack(taps, 1), LC.OCC_BYTES, n * LC.OCC_BYTES, tail=8)
    print(f"occupancy {kind}: largest tap offset {top} of {n * 4} bytes (x-row index up to {int(torch.stack(taps, 1).max()) // W}), "
          f"{int(same.sum())} of {len(pts)} points compared, {100 * float(keep.double().mean()):.0f} % kept")
    assert tail and float(same.double().mean()) >= 0.9 and bool(same[:2].all()) and 0.2 <= float(keep.double().mean()) <= 0.8
    assert int(torch.stack(taps, 1).max()) // W >= (D * H - 1) - 1
    q = fm.query_points(fr, pts.to(DEV), occ_cull=True, want=("rgb", "sigma"))["raw"]
    r = fm.render_fused(fr, LC.point_rays(pts), 1, occ_cull=True, want=("raw",))["raw"].reshape(-1, 4)
    assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(r).all())
    kept = (q[:, :3] != 0).any(1).cpu()                    # a kept point's colours are sigmoids; a culled point's row is zero
    assert not bool(q[~kept.to(DEV)].any())
    wrong = int(((kept != keep) & same).sum())
    # the renderer also zeroes the colours of a kept sample whose alpha is at most 1e-14 (demo_render.py's valid1), so its rows are
    # compared with the query's: zero where the reference culls, the query's density and -- where that is well above 0 -- colours
    cmp = same.to(DEV)
    culled_rows = r[cmp & ~keep.to(DEV)]
    dense = cmp & keep.to(DEV) & (q[:, 3] > 1e-3)
    e_sigma = float((r[:, 3] - q[:, 3])[cmp].abs().max())
    e_rgb = float((r[:, :3] - q[:, :3])[dense].abs().max())
    print(f"occupancy {kind}: {wrong} keep / cull decisions of query_points differ from the reference; render_fused against the query: "
          f"sigma max-abs {e_sigma:.2e}, rgb max-abs {e_rgb:.2e} on {int(dense.sum())} kept points with density (bound {TOL_RAW:.0e})")
    assert wrong == 0
    assert not bool(culled_rows.any()) and int(dense.sum()) >= len(pts) // 16 and e_sigma <= TOL_RAW and e_rgb <= TOL_RAW
    del fr, vol, own
    LC.release()


# ---- the producers of the large tensors ------------------------------------------------------------------------------------------------
def _equal_in_slices(dst, src_of, n, step):
    for i in range(0, n, step):
        if not torch.equal(dst[i:i + step], src_of(i, min(n, i + step))):
            return False
    return True


def test_relayout_volume_at_the_limit(fm):
    D, H, W = LC.level_shape("rows", VOXEL_BYTES)
    need(2 * D * H * W * VOXEL_BYTES + (2 << 30))
    src = LC.big_rand((CH, D, H, W), seed=400)
    dst = torch.empty((D, H, W, CH), device=DEV)
    fm.L.check(fm.L.lib().gpnerf_relayout_volume(src.data_ptr(), dst.data_ptr(), D, H, W, None), "gpnerf_relayout_volume")
    torch.cuda.synchronize()
    print(f"relayout_volume: [{D}, {H}, {W}, {CH}] {dst.numel() * 4} bytes")
    assert dst.numel() * 4 == LIM_BYTES - 256
    assert _equal_in_slices(dst, lambda a, b: src[:, a:b].permute(1, 2, 3, 0), D, 256)
    del src, dst
    LC.release()


def test_relayout_featmaps_at_the_limit(fm):
    h, w = LC.map_shape("rows", VOXEL_BYTES)
    need(2 * h * w * VOXEL_BYTES + (2 << 30))
    src = LC.big_rand((1, CH, h, w), seed=401)
    dst = torch.empty((1, h, w, CH), device=DEV)
    fm.L.check(fm.L.lib().gpnerf_relayout_featmaps(src.data_ptr(), dst.data_ptr(), 1, h, w, None), "gpnerf_relayout_featmaps")
    torch.cuda.synchronize()
    print(f"relayout_featmaps: [1, {h}, {w}, {CH}] {dst.numel() * 4} bytes")
    assert dst.numel() * 4 == LIM_BYTES - 256
    assert _equal_in_slices(dst[0], lambda a, b: src[0, :, a:b].permute(1, 2, 0), h, 1 << 20)
    del src, dst
    LC.release()


def test_relayout_images_at_the_limit(fm):
    H, W = LC.map_shape("row_bytes", PIXEL_BYTES)
    need(H * W * (PIXEL_BYTES + 12) + (2 << 30))
    src = LC.big_rand((1, 3, H, W), seed=402)
    dst = fm.relayout_images(src)
    torch.cuda.synchronize()
    print(f"relayout_images: [1, {H}, {W}, 4] {dst.numel() * 4} bytes")
    assert dst.numel() * 4 == LIM_BYTES - 4096 and W * PIXEL_BYTES == LIM24 - 16
    # de-normalised (x * 0.5 is exact, so the fused and the two-step form round alike), the fourth channel zero
    assert _equal_in_slices(dst[0, :, :, :3], lambda a, b: src[0, :, a:b].permute(1, 2, 0) * 0.5 + 0.5, H, 16)
    assert not bool(dst[0, :, :, 3].any())
    del src, dst
    LC.release()


# ---- per-sample output rows beyond 2^31 bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["reference-order", "split-f16"])
def test_per_sample_rows_beyond_2_31_bytes(split, fm, syn):
    """One frame of 2^20 + 33 rays x 128 samples with raw, weights and z_vals: `raw` is 2 GiB + 66 KiB.  The first 64 rays, the last
    97 and the 64 around the row at which raw's byte offset crosses 2^31, rendered alone, must give the same rows: per-sample outputs
    do not depend on the tiling (include/gpnerf_hip.h on ray_order), so raw and z_vals are bit-equal, and weights are where both
    launches are unsplit (fm.render_plan) and within the header's 1e-6 for split composites otherwise."""
    N, S = (1 << 20) + 33, 128
    assert N * S * 16 == HALF + 66 * 1024
    need(N * S * 24 + (4 << 30))
    sc = syn.make_scene(H=16, W=16, seed=7, aabb_half=(0.2, 0.3, 0.12), pose="random", bias_std=0.1, sigma_bias=0.5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    fr = fm.Frame(dev(sc["src_imgs"][0]), dev(sc["featmaps"]), [dev(v) for v in sc["volumes"]], dev(sc["src_Ks"][0]), dev(sc["src_poses"][0]),
                  sc["Rh"][0], sc["Th"][0], sc["bounds"][0, 0], sc["voxel_size"], sc["out_sh"][0], fm.pack_head(sc["head"], torch.device(DEV)))
    base = dev(np.concatenate([sc["ray_o"][0], sc["ray_d"][0], sc["near"][0][:, None], sc["far"][0][:, None]], 1).astype(np.float32))
    i = torch.arange(N, device=DEV)
    rays = base[i % base.shape[0]].contiguous()
    rays[:, 7] += (i % 13).float() * 1e-3               # neighbouring copies of a ray are not the same ray
    want = ("raw", "weights", "z_vals")
    big = fm.render_fused(fr, rays, S, want=want, split_f16=split)
    assert big["raw"].numel() * 4 > HALF and float(big["weights"].max()) > 0
    cross = HALF // (S * 16)
    worst = 0.0
    for a, b in ((0, 64), (N - 97, N), (cross - 32, cross + 32)):
        small = fm.render_fused(fr, rays[a:b].contiguous(), S, want=want, split_f16=split)
        for k in ("raw", "z_vals"):
            assert torch.equal(bits(big[k][a:b]), bits(small[k])), (k, a, b)
        unsplit = all(fm.render_plan(fr, n, S, want=want, split_f16=split).split == 1 for n in (N, b - a))
        err = float((big["weights"][a:b] - small["weights"]).abs().max())
        worst = max(worst, err)
        assert float(small["weights"].max()) > 0
        if unsplit:
            assert torch.equal(bits(big["weights"][a:b]), bits(small["weights"])), (a, b)
        else:
            assert err <= 1e-6, (a, b, err)
    print(f"rows beyond 2^31 ({'split-f16' if split else 'reference-order'}): raw {big['raw'].numel() * 4} bytes, rays [{cross - 32}, {cross + 32}) "
          f"straddle the crossing; raw and z_vals bit-equal, weights max-abs {worst:.1e}")
    del big, rays, fr
    LC.release()
