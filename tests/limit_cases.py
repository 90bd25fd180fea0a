"""Helpers of test_gpu_limits.py: the extreme shapes include/gpnerf_hip.h still accepts, re-derived from its limits; query points on
which float32 evaluates F.grid_sample's index rule exactly; and a plain-torch float64 reference of the gathers (no project code).

The limits (to_framek() in gpnerf_kernels.hip, promised by the header): every tensor below 2^32 bytes, every x-row below 2^24 bytes,
every row count (D*H, img_h, feat_h) below 2^24; a folded level (256 bytes per voxel) below 2^32 bytes with x-rows below 2^24 bytes.

Why the points sit on a lattice.  The kernels follow ATen: the continuous index ((g + 1) / 2) * (size - 1) is a float32 value, and on
an axis of 2^17 or 2^24 entries float32 resolves it to 1/128 of a voxel, or to a whole row.  A float64 evaluation of the same rule
agrees with that only where the float32 evaluation is exact, so every checked point is k / 2^b per axis with b chosen from the axis'
size such that each intermediate of the rule fits 24 bits (lattice_bits).  The test asserts that condition on its inputs (the float32
and the float64 index of every compared point agree to 5e-7 of a voxel): a condition on the points, not on the code under test.  The
points one ulp around g = +-1 run everywhere and are compared where they meet it (the short axes; always at g = -1, where g + 1 is
exact)."""
import numpy as np
import torch

DEV = "cuda:0"
LIM_BYTES = 1 << 32
LIM24 = 1 << 24
HALF = 1 << 31
CH = 32
VOXEL_BYTES, FOLDED_BYTES, PIXEL_BYTES, OCC_BYTES = CH * 4, CH * 8, 16, 4
TOL_FEAT = 2e-6            # gathered features, x max|value| = 1: test_stage_entry_points_match_reference_golden's bound on st_vol_feat
TOL_RAW = 1e-4             # test_gpu_field.py's TOL on st_raw
INDEX_SLACK = 5e-7         # |float64 index - float32 index| summed over a point's axes, in voxels: at most 2 x that x max|value| = 1e-6
                           # of reference error, half of TOL_FEAT (lattice points: 0)
VIEW_SHIFT_X = (1, 2, 0)   # view v maps p_x in [0, 2] to [0, (W - 1) * 2^(1 - shift)]: a different (s_x, s_y) per view
VIEW_SHIFT_Y = (1, 0, 2)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
def level_accepted(D, H, W, cell=VOXEL_BYTES):
    """the header's rule for a volume level of `cell` bytes per voxel (128; 256 for a level that is also folded)"""
    return D * H * W * cell < LIM_BYTES and D * H < LIM24 and W * cell < LIM24 and D * H * W * VOXEL_BYTES < LIM_BYTES and W * VOXEL_BYTES < LIM24


def map_accepted(h, w, cell):
    """the header's rule for one view's feature map (128 bytes per pixel) or image (16)"""
    return h * w * cell < LIM_BYTES and w * cell < LIM24 and h < LIM24


def level_shape(kind, cell):
    """(D, H, W) of the extreme level: kind "rows" = the most x-rows of two voxels (D a round depth, H what the limits leave),
    "row_bytes" = the longest x-row (16 x 16 of them)"""
    if kind == "rows":
        W = 2
        rows = min(LIM24 - 1, (LIM_BYTES - 1) // (W * cell))
        D = 4095 if cell == VOXEL_BYTES else 2048
        shape = (D, rows // D, W)
    else:
        shape = (16, 16, (LIM24 - 1) // cell)
    D, H, W = shape
    assert level_accepted(D, H, W, cell) and not level_accepted(D, H + 1, W, cell) and not level_accepted(D, H, W + 1, cell), shape
    return shape


def map_shape(kind, cell):
    """(h, w) of the extreme per-view map"""
    if kind == "rows":
        h = LIM24 - 1
        w = (LIM_BYTES - 1) // (h * cell)
    else:
        w = (LIM24 - 1) // cell
        h = (LIM_BYTES - 1) // (w * cell)
    assert map_accepted(h, w, cell) and not map_accepted(h + 1, w, cell) and not map_accepted(h, w + 1, cell), (h, w)
    return h, w


def total_memory():
    return torch.cuda.get_device_properties(0).total_memory


def big_rand(shape, seed):
    """torch.rand(shape) * 2 - 1 on the device, slice by slice of the first dimension and in place (no second tensor of that size):
    position-dependent values, so a wrapped or truncated offset reads a different number"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.empty(shape, device=DEV, dtype=torch.float32)
    step = max(1, (1 << 28) // max(1, t[0].numel()))
    for i in range(0, shape[0], step):
        s = t[i:i + step]
        s.copy_(torch.rand(s.shape, device=DEV, generator=g))
        s.mul_(2).sub_(1)
    return t


def release(*tensors):
    del tensors
    torch.cuda.empty_cache()


# ---- the frame under test ------------------------------------------------------------------------------------------------------------
def small_frame(fm, syn, seed=5):
    """An ordinary 16 x 16 frame with 2 x 2 x 2 levels and the exact geometry: Rh = I, Th = 0, bounds_min = 0, voxel = 1,
    out_sh = (2, 2, 2), so g = p - 1; proj[v] = rows (s_x, 0, 0, 0), (0, s_y, 0, 0), (0, 0, 0, 1), so u = s_x p_x, w = s_y p_y, h_z = 1."""
    sc = syn.make_scene(H=16, W=16, seed=seed, make_volumes=False, bias_std=0.1, sigma_bias=0.5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    vols = [torch.rand((CH, 2, 2, 2), device=DEV, generator=g) * 2 - 1 for _ in range(4)]
    blob = fm.pack_head(sc["head"], torch.device(DEV))
    fr = fm.Frame(dev(sc["src_imgs"][0]), dev(sc["featmaps"]), vols, dev(sc["src_Ks"][0]), dev(sc["src_poses"][0]), np.eye(3, dtype=np.float32),
                  np.zeros(3, np.float32), np.zeros(3, np.float32), np.ones(3, np.float32), np.array([2, 2, 2], np.int32), blob)
    fr.c.Rh[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    for a in range(3):
        fr.c.Th[a], fr.c.bounds_min[a], fr.c.voxel[a], fr.c.out_sh[a] = 0.0, 0.0, 1.0, 2
    set_proj(fr)
    return fr, blob, sc


def same_taps(g32, size):
    """whether float32 and float64 give the axis the same live taps at g32: the same floor and the same verdict on a zero fraction
    (a keep / cull decision over a non-negative volume depends on which taps carry weight, not on the weights)"""
    ix = ((g32.double() + 1) / 2) * (size - 1)
    ix32 = (((g32 + 1) / 2) * float(size - 1)).double()
    return (torch.floor(ix) == torch.floor(ix32)) & ((ix == torch.floor(ix)) == (ix32 == torch.floor(ix32)))


def view_scales(fr):
    """(s_x, s_y) of every view for the frame's current image size: (size - 1) * 2^-shift, exact in float32"""
    return [((fr.c.img_w - 1) * 2.0 ** -VIEW_SHIFT_X[v], (fr.c.img_h - 1) * 2.0 ** -VIEW_SHIFT_Y[v]) for v in range(3)]


def set_proj(fr):
    for v, (sx, sy) in enumerate(view_scales(fr)):
        assert float(np.float32(sx)) == sx and float(np.float32(sy)) == sy
        fr.c.proj[v][:] = [sx, 0, 0, 0, 0, sy, 0, 0, 0, 0, 0, 1]


def swap_level(fr, l, vol):
    """level l of the frame becomes `vol` [D, H, W, 32] (pointer and sizes; the tensor stays alive on the frame)"""
    fr.vols[l] = vol
    fr.c.vol[l] = vol.data_ptr()
    for a in range(3):
        fr.c.vol_dhw[l][a] = vol.shape[a]
    fr.vols_folded, fr._folded_valid = None, False
    for k in range(len(fr.vols)):
        fr.c.vol_folded[k] = None


def swap_featmaps(fr, maps):
    fr.featmaps = maps
    fr.c.featmaps, fr.c.feat_h, fr.c.feat_w = maps.data_ptr(), maps.shape[1], maps.shape[2]


def swap_images(fr, imgs):
    fr.imgs = imgs
    fr.c.imgs, fr.c.img_h, fr.c.img_w = imgs.data_ptr(), imgs.shape[1], imgs.shape[2]
    set_proj(fr)


def point_rays(pts):
    """zero-length rays at the points: with S = 1 a ray's only sample is its origin"""
    rays = torch.zeros((pts.shape[0], 8), dtype=torch.float32)
    rays[:, :3] = pts
    return rays.to(DEV)


# ---- query points --------------------------------------------------------------------------------------------------------------------
def lattice_bits(*sizes):
    """b such that p = k / 2^b, k <= 2^(b + 1), makes (p / 2^j) * (size - 1) exact in float32 for every size: k's bits plus the bits of
    the odd part of size - 1 stay within 24"""
    b = 12
    for n in sizes:
        m = n - 1
        while m > 1 and m % 2 == 0:
            m //= 2
        b = min(b, 23 - max(1, m).bit_length())
    assert b >= 0
    return b


def _axis_draw(rng, n, bits, upper):
    """n lattice coordinates in [0, 2]; upper: in [1, 2] (the far half of the axis)"""
    lo = (1 << bits) if upper else 0
    return rng.integers(lo, (2 << bits) + 1, n).astype(np.float64) / float(1 << bits)


def make_points(bits_xyz, outer, n_fill=3000, seed=0):
    """Points p [P, 3] (float32, on the host) for axes whose lattices have bits_xyz bits.  `outer` is the axis (0 = x, 1 = y, 2 = z)
    whose index multiplies the largest stride: three quarters of the fill lie in its far half, so that more than half of all points
    have a tap beyond 2^31 bytes.  First: the first voxel, the last voxel, 64 points of the last row (every other axis at its end),
    the points one float32 step inside and outside p = 0 and p = 2 (g = -1 and g = +1) on every axis; then the random fill."""
    rng = np.random.default_rng(seed)
    far = lambda n, a: _axis_draw(rng, n, bits_xyz[a], True)
    pts = [np.zeros((1, 3)), np.full((1, 3), 2.0)]
    last_row = np.full((64, 3), 2.0)
    last_row[:, 0] = _axis_draw(rng, 64, bits_xyz[0], False)
    pts.append(last_row)
    two = np.float32(2.0)
    edge = [np.float32(2.0 ** -24), -np.float32(2.0 ** -23), np.nextafter(two, np.float32(0)), np.nextafter(two, np.float32(3))]
    for a in range(3):
        for e in edge:
            q = np.stack([far(8, 0), far(8, 1), far(8, 2)], 1)
            q[:, a] = float(e)
            pts.append(q)
    fill = np.stack([_axis_draw(rng, n_fill, bits_xyz[a], False) for a in range(3)], 1)
    n_far = (3 * n_fill) // 4
    fill[:n_far, outer] = far(n_far, outer)
    pts.append(fill)
    p = np.concatenate(pts, 0)
    p32 = p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p)
    return torch.from_numpy(p32)


# ---- the reference: plain torch, float64 ---------------------------------------------------------------------------------------------
def axis_taps(g32, size):
    """F.grid_sample's align-corners rule ((g + 1) / 2) * (size - 1) in float64 on the float32 coordinate g32 [P] (host), zero padding:
    tap indices [P, 2] (int64, 0 where a tap is out of range), weights [P, 2] (float64, 0 there), and how far the float32 evaluation
    of the same rule lies from it, in voxels"""
    ix = ((g32.double() + 1) / 2) * (size - 1)
    ix32 = ((g32 + 1) / 2) * float(size - 1)
    assert ix32.dtype == torch.float32
    j0 = torch.floor(ix)
    t = ix - j0
    j = torch.stack([j0, j0 + 1], 1)
    w = torch.stack([1 - t, t], 1)
    ok = (j >= 0) & (j < size) & torch.isfinite(j)
    zero = torch.zeros_like(w)
    return torch.where(ok, j, zero).long(), torch.where(ok, w, zero), (ix - ix32.double()).abs()


def ref_volume(vol, g32):
    """trilinear sample of vol [D, H, W, C] (device) at g32 [P, 3] (x, y, z; host float32): values [P, C] float64 (device), the
    voxel index of every live tap [P, 8] (int64 host, -1 for a tap with no weight), the points' index slack [P]"""
    D, H, W, C = vol.shape
    (jx, wx, sx), (jy, wy, sy), (jz, wz, sz) = axis_taps(g32[:, 0], W), axis_taps(g32[:, 1], H), axis_taps(g32[:, 2], D)
    flat = vol.view(-1, C)
    out = torch.zeros((g32.shape[0], C), dtype=torch.float64, device=vol.device)
    taps = []
    for a in range(2):
        for b in range(2):
            for e in range(2):
                w = wz[:, a] * wy[:, b] * wx[:, e]
                lin = (jz[:, a] * H + jy[:, b]) * W + jx[:, e]
                out += flat[lin.to(vol.device)].double() * w.to(vol.device)[:, None]
                taps.append(torch.where(w > 0, lin, torch.full_like(lin, -1)))
    return out, torch.stack(taps, 1), sx + sy + sz


def ref_bilinear(img, gx32, gy32):
    """bilinear sample of img [h, w, C] (device): values [P, C] float64, live tap pixel indices [P, 4], slack [P]"""
    h, w, C = img.shape
    (jx, wx, sx), (jy, wy, sy) = axis_taps(gx32, w), axis_taps(gy32, h)
    flat = img.view(-1, C)
    out = torch.zeros((gx32.shape[0], C), dtype=torch.float64, device=img.device)
    taps = []
    for b in range(2):
        for e in range(2):
            wt = wy[:, b] * wx[:, e]
            lin = jy[:, b] * w + jx[:, e]
            out += flat[lin.to(img.device)].double() * wt.to(img.device)[:, None]
            taps.append(torch.where(wt > 0, lin, torch.full_like(lin, -1)))
    return out, torch.stack(taps, 1), sx + sy


def ref_views(imgs, maps, scales, pts):
    """Projector.compute on the exact geometry: u = s_x p_x, w = s_y p_y in float32, clamped to +-1e6; in image and in front (h_z = 1)
    -> mask; bilinear rgb from imgs [V, H, W, 4] and 32 channels from maps [V, h, w, 32] at the normalised 2 u / (W - 1) - 1.
    Returns feat [P, V, 35] float64 (device), mask [P, V] float32 (host), the live taps of the images [P, V, 4] and of the maps
    [P, V, 4] (pixel index inside the view, -1 for none), the slack [P, V]."""
    V, H, W, _ = imgs.shape
    feats, masks, itaps, ftaps, slack = [], [], [], [], []
    for v in range(V):
        sx, sy = scales[v]
        u = (pts[:, 0] * float(np.float32(sx))).clamp(-1e6, 1e6)
        w = (pts[:, 1] * float(np.float32(sy))).clamp(-1e6, 1e6)
        assert u.dtype == torch.float32
        masks.append(((u <= W - 1) & (u >= 0) & (w <= H - 1) & (w >= 0)).float())
        nx, ny = 2.0 * u / float(W - 1) - 1.0, 2.0 * w / float(H - 1) - 1.0
        rgb, it, s_i = ref_bilinear(imgs[v], nx, ny)
        f, ft, s_f = ref_bilinear(maps[v], nx, ny)
        feats.append(torch.cat([rgb[:, :3], f], 1))
        itaps.append(it); ftaps.append(ft); slack.append(torch.maximum(s_i, s_f))
    return torch.stack(feats, 1), torch.stack(masks, 1), torch.stack(itaps, 1), torch.stack(ftaps, 1), torch.stack(slack, 1)


def reach(taps, cell, nbytes, tail=256):
    """What the reference's own live taps reach: (largest byte offset, share of points with a tap at or beyond 2^31, whether a tap
    lies in the tensor's last `tail` bytes).  taps [P, ...] element indices (-1 = none), cell = bytes per element."""
    off = taps.reshape(taps.shape[0], -1) * cell
    top = int(off.max())
    share = float((off >= HALF).any(1).double().mean())
    return top, share, bool(top >= nbytes - tail and top < nbytes)
