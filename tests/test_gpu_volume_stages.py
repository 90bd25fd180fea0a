"""The sparse volume builder (csrc/gpnerf_volume.hip) stage by stage, off the path the end-to-end tests take: voxels crowded enough
to scan, the coarse-site builder on its own, the convolution forms at the widths the pyramid never uses, device-side row counts, the
scatter launch, the host caches of volume.py and rows outside the grid -- each against the restatements of tests/volume_cases.py
(pinned on the CPU by tests/test_volume_stages_host.py).  Tolerances come from vc.bound: the same formula in float32 on the CPU."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import volume_cases as vc
from oracle import producers_ref as pref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I3 = C.c_int32 * 3
SENTINEL = 0x5A5A5A5A


def _L():
    L = importlib.import_module("gp-nerf_amd._lib")
    return L, L.lib()


def _vol():
    return importlib.import_module("gp-nerf_amd.volume")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _index(L, lib, coords, dims):
    cd = _t(coords)
    grid = torch.empty(dims, device=DEV, dtype=torch.int32)
    L.check(lib.gpnerf_sparse_index(cd.data_ptr(), None, len(coords), I3(*dims), grid.data_ptr(), None), "index")
    return cd, grid


# ---- 1. crowded voxels ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crowd():
    dims = (8, 16, 8)
    coords, planted = vc.crowded(21)
    return dims, coords, planted, vc.companions(coords, dims)


def test_the_index_grid_holds_the_highest_row_of_a_voxel(crowd):
    dims, coords, _, _ = crowd
    L, lib = _L()
    _, grid = _index(L, lib, coords, dims)
    assert np.array_equal(grid.cpu().numpy(), vc.index_grid(coords, dims))


@pytest.mark.parametrize("channels", [32, 16, 5])
def test_merge_duplicates_adds_in_its_documented_order_bit_for_bit(crowd, channels):
    """Owners with 1, 7 and 8 companions take the slot path (8 = every slot, a full sorting network), 9 and more the scan, 64 / 65
    companions straddle its chunks: the owner's value first, then the others in ascending row order, exactly."""
    dims, coords, planted, comp = crowd
    L, lib = _L()
    m = len(coords)
    feat = np.random.default_rng(channels).standard_normal((m, channels)).astype(np.float32)
    want, count = vc.merge_ordered(feat, coords, dims)
    cd, grid = _index(L, lib, coords, dims)
    fd = _t(feat)
    scratch = torch.full(((1 + vc.DUP_SLOTS) * m,), SENTINEL, device=DEV, dtype=torch.int32)
    L.check(lib.gpnerf_sparse_merge_duplicates(fd.data_ptr(), channels, cd.data_ptr(), grid.data_ptr(), m, I3(*dims), scratch.data_ptr(), None), "merge")
    torch.cuda.synchronize()
    got, sc = fd.cpu().numpy(), scratch.cpu().numpy()
    owners = sorted(comp)
    rest = np.setdiff1d(np.arange(m), owners)
    assert np.array_equal(got[rest].view(np.uint32), feat[rest].view(np.uint32)), "a row that owns no shared voxel changed"
    for o in owners:
        assert np.array_equal(got[o].view(np.uint32), want[o].view(np.uint32)), (o, int(count[o]), np.abs(got[o] - want[o]).max())
    assert np.array_equal(sc[:m], count)
    slots = sc[m:].reshape(m, vc.DUP_SLOTS)
    assert (slots[rest] == SENTINEL).all()
    unsorted = sum(1 for o in owners if count[o] <= vc.DUP_SLOTS and slots[o, :count[o]].tolist() != sorted(slots[o, :count[o]].tolist()))
    print(f"merge, {channels} channels: {unsorted} of the {sum(count[o] <= vc.DUP_SLOTS for o in owners)} slot-path owners found their slots out of order")
    for o in owners:
        n = min(int(count[o]), vc.DUP_SLOTS)
        assert set(slots[o, :n].tolist()) <= set(comp[o]) and len(set(slots[o, :n].tolist())) == n and (slots[o, n:] == SENTINEL).all()


def _levels_vs_float64(net, code, coords, dims, label):
    """dense_levels_hip against oracle/producers_ref.dense_levels in float64; the bound from the same restatement in float32"""
    coord4 = torch.cat([torch.zeros((len(coords), 1), dtype=torch.long), torch.from_numpy(coords).long()], 1)
    with torch.no_grad():
        want32 = pref.dense_levels(net, code, coord4, dims)
        net = net.to(DEV)
        hip = [v.cpu() for v in net.dense_levels_hip(code.to(DEV), coord4.to(DEV), list(dims))]
        net = net.cpu().double()
        want = pref.dense_levels(net, code.double(), coord4, dims)
        net.float()
    assert len(hip) == len(want)
    for lv, (a, b, b32) in enumerate(zip(hip, want, want32)):
        ref = b[0].permute(1, 2, 3, 0).numpy()
        lim = vc.bound(ref, b32[0].permute(1, 2, 3, 0).numpy())
        err = float(np.abs(a.numpy().astype(np.float64) - ref).max())
        print(f"{label} level {lv + 1}: error {err:.3e}, bound {lim:.3e}, ratio {err / lim:.3f}, {int((ref != 0).any(-1).sum())} sites")
        assert a.shape == ref.shape and err <= lim, (label, lv, err, lim)
        assert (ref != 0).any()
    return hip


@pytest.mark.parametrize("in_dim", [32, 16, 12])
def test_a_one_level_net_on_crowded_voxels_is_the_float64_rulebook(in_dim):
    """subm_shared_rows_kernel (no entry point of its own) and pyramid_run's vertex level: owners of voxels with up to 139 companions,
    neighbours of each other, at the split form's widths and the VALU form's"""
    dims = (16, 32, 16)                                      # (the builder takes grids that are multiples of 16)
    coords, _ = vc.crowded(31 + in_dim, dims, 450)
    net = vc.random_net(_vol(), 1, in_dim, [32], 100 + in_dim)
    code = torch.randn((len(coords), in_dim), generator=torch.Generator().manual_seed(in_dim))
    _levels_vs_float64(net, code, coords, dims, f"crowded one-level net, in_dim {in_dim}")


def _run_conv(L, lib, form, coords, feat, w, scale, shift, oc, dims, strided, m_dev=None, feat_dev=None):
    """one convolution by its public entry point; `out` starts as NaN.  form: valu (gpnerf_sparse_conv3), mfma (.._mfma), split (.._mfma16)"""
    cin, cout = w.shape[1], w.shape[2]
    cd, grid = _index(L, lib, coords, dims)
    fd = _t(feat) if feat_dev is None else feat_dev
    ocd, sc, sh = _t(oc), _t(scale), _t(shift)
    out = torch.full((len(oc), cout), float("nan"), device=DEV)
    md = None if m_dev is None else torch.tensor([m_dev], device=DEV, dtype=torch.int32)
    mp = None if md is None else md.data_ptr()
    if form == "valu":
        wp = _t(w)
        fn = lib.gpnerf_sparse_conv3
    elif form == "mfma":
        packed = np.zeros(int(lib.gpnerf_sparse_packed_weight_floats(cin)), np.float32)
        L.check(lib.gpnerf_sparse_pack_weight(w.ctypes.data_as(L.FP), cin, cout, packed.ctypes.data_as(L.FP)), "pack")
        wp, fn = _t(packed), lib.gpnerf_sparse_conv3_mfma
    else:
        packed = np.zeros(int(lib.gpnerf_sparse_packed_weight16_bytes(cin)), np.uint8)
        L.check(lib.gpnerf_sparse_pack_weight16(w.ctypes.data_as(L.FP), cin, cout, packed.ctypes.data_as(C.c_void_p)), "pack16")
        wp, fn = _t(packed), lib.gpnerf_sparse_conv3_mfma16
    L.check(fn(int(strided), fd.data_ptr(), cin, grid.data_ptr(), I3(*dims), ocd.data_ptr(), mp, len(oc), wp.data_ptr(), cout,
               sc.data_ptr(), sh.data_ptr(), out.data_ptr(), None), form)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("cin,form", [(12, "valu"), (16, "split"), (24, "mfma")])
def test_conv_through_the_merged_grid_is_the_rulebook_where_the_own_voxel_is_not_shared(cin, form):
    """The claim in subm_shared_rows_kernel's comment, by public entry points only: index, a copy, merge_duplicates, a convolution --
    every row that has its voxel to itself then holds spconv's rulebook value (its neighbours' voxel SUMS through the owners)."""
    dims = (8, 16, 8)
    coords, planted = vc.crowded(41 + cin)
    L, lib = _L()
    m, cout = len(coords), 32
    g = np.random.default_rng(cin)
    feat = g.standard_normal((m, cin)).astype(np.float32)
    w = (g.standard_normal((27, cin, cout)) * 0.1).astype(np.float32)
    scale, shift = g.uniform(0.5, 1.5, cout).astype(np.float32), (g.standard_normal(cout) * 0.2).astype(np.float32)
    cd, grid = _index(L, lib, coords, dims)
    merged = _t(feat).clone()
    scratch = torch.empty(((1 + vc.DUP_SLOTS) * m,), device=DEV, dtype=torch.int32)
    L.check(lib.gpnerf_sparse_merge_duplicates(merged.data_ptr(), cin, cd.data_ptr(), grid.data_ptr(), m, I3(*dims), scratch.data_ptr(), None), "merge")
    got = _run_conv(L, lib, form, coords, None, w, scale, shift, coords, dims, False, feat_dev=merged)

    def rulebook(dtype):
        x = pref.SparseTensor(torch.from_numpy(feat).to(dtype), torch.from_numpy(coords).long(), dims)
        y = pref.subm_conv3d_rulebook(x, torch.from_numpy(w).to(dtype).view(3, 3, 3, cin, cout)).features
        return torch.relu(y * torch.from_numpy(scale).to(dtype) + torch.from_numpy(shift).to(dtype)).numpy()

    ref, same32 = rulebook(torch.float64), rulebook(torch.float32)
    shared = np.array([tuple(c) in planted for c in coords.tolist()])
    alone = ~shared
    near = np.array([any(np.abs(np.array(p) - c).max() == 1 for p in planted) for c in coords])
    assert alone.sum() == 150 and (alone & near).sum() >= 5, "rows beside a crowded voxel are what this is about"
    lim = vc.bound(ref[alone], same32[alone])
    err = float(np.abs(got[alone] - ref[alone]).max())
    print(f"merged-grid convolution, {form} cin {cin}: error {err:.3e}, bound {lim:.3e}, ratio {err / lim:.3f}")
    assert err <= lim
    # and the rows of a shared voxel are NOT the rulebook's here: the kernel that recomputes them has something to do
    assert np.abs(got[shared] - ref[shared]).max() > 1e-2


# ---- 2. coarse sites -----------------------------------------------------------------------------------------------------------------
def _down_sites(L, lib, coords, out_dims, m_dev=None, cap=None, rows_alloc=None):
    cd = _t(coords)
    cells = int(np.prod(out_dims))
    cap = cells if cap is None else cap
    rows_alloc = max(cap, 1) if rows_alloc is None else rows_alloc
    grid = torch.full(out_dims, SENTINEL, device=DEV, dtype=torch.int32)
    oc = torch.full((rows_alloc, 3), SENTINEL, device=DEV, dtype=torch.int32)
    om = torch.full((1,), SENTINEL, device=DEV, dtype=torch.int32)
    md = None if m_dev is None else torch.tensor([m_dev], device=DEV, dtype=torch.int32)
    L.check(lib.gpnerf_sparse_down_sites(cd.data_ptr(), None if md is None else md.data_ptr(), len(coords), I3(*out_dims), grid.data_ptr(),
                                         oc.data_ptr(), om.data_ptr(), cap, None), "down_sites")
    torch.cuda.synchronize()
    return grid.cpu().numpy(), oc.cpu().numpy(), int(om.cpu()[0])


def _check_sites(grid, oc, n, want, out_dims):
    """m_out exact; the rows a permutation of the wanted sites; grid[cell] == r exactly where coords[r] is that cell; -1 elsewhere"""
    assert n == len(want)
    rows = oc[:n].astype(np.int64)
    assert sorted(map(tuple, rows.tolist())) == list(map(tuple, want.tolist()))
    expect = -np.ones(out_dims, np.int64)
    expect[rows[:, 0], rows[:, 1], rows[:, 2]] = np.arange(n)
    assert np.array_equal(grid, expect)
    assert (oc[n:] == SENTINEL).all()


def _site_rows(out_dims, m, seed):
    g = np.random.default_rng(seed)
    return np.stack([g.integers(0, 2 * n, m) for n in out_dims], 1).astype(np.int32)


@pytest.mark.parametrize("out_dims,m", [((8, 16, 8), 256), ((16, 40, 24), 2500), ((9, 25, 11), 600)])
def test_down_sites_gives_every_reachable_coarse_site_one_row(out_dims, m):
    """assign_kernel with one partial workgroup (1 024 cells), 3.75 workgroups (15 360) and odd sizes (2 475); the scan over its four
    wavefronts decides which row a cell gets, so a fault there shows as a row used twice or a hole in the grid"""
    L, lib = _L()
    coords = _site_rows(out_dims, m, m)
    want = vc.reachable_sites(coords, out_dims)
    assert 0 < len(want) < int(np.prod(out_dims))
    grid, oc, n = _down_sites(L, lib, coords, out_dims)
    _check_sites(grid, oc, n, want, out_dims)


def test_down_sites_reads_no_row_past_the_device_row_count():
    L, lib = _L()
    out_dims, m = (16, 40, 24), 2500
    coords = _site_rows(out_dims, m, 77)
    m_dev = int(0.6 * m)
    head = vc.reachable_sites(coords[:m_dev], out_dims)
    both = vc.reachable_sites(coords, out_dims)
    assert len(both) > len(head) + 100, "the rows past the count would mark sites of their own"
    grid, oc, n = _down_sites(L, lib, coords, out_dims, m_dev=m_dev)
    _check_sites(grid, oc, n, head, out_dims)
    # a count beyond the capacity is clamped to it
    grid, oc, n = _down_sites(L, lib, coords[:m_dev], out_dims, m_dev=m + 1000)
    _check_sites(grid, oc, n, head, out_dims)


def test_down_sites_with_fewer_rows_than_sites_stays_inside_its_buffers():
    """m_out_cap below the reachable count: rows below the cap are consistent with the grid, the cells that got no row are inactive
    (-1, none left marked), nothing is written past coords[3 * cap], and *m_out counts every site -- which is why every kernel
    downstream clamps its row count with min(*m, cap)."""
    L, lib = _L()
    out_dims, m = (16, 40, 24), 2500
    coords = _site_rows(out_dims, m, 78)
    want = vc.reachable_sites(coords, out_dims)
    cap = len(want) // 2 + 3
    grid, oc, n = _down_sites(L, lib, coords, out_dims, cap=cap, rows_alloc=len(want) + 8)
    assert n >= cap and n == len(want)
    assert (oc[cap:] == SENTINEL).all()
    rows = oc[:cap].astype(np.int64)
    assert len({tuple(r) for r in rows.tolist()}) == cap and {tuple(r) for r in rows.tolist()} <= {tuple(r) for r in want.tolist()}
    expect = -np.ones(out_dims, np.int64)
    expect[rows[:, 0], rows[:, 1], rows[:, 2]] = np.arange(cap)
    assert np.array_equal(grid, expect) and grid.min() == -1


# ---- 3. the convolution forms ----------------------------------------------------------------------------------------------------------
CONV_DIMS = (16, 32, 16)
CONV_SITES = 1000
WORST = {}                                                 # form -> worst error / bound seen in this run (printed, DESIGN.md 4.2 records them)
FORM_CASES = [("mfma", 8, 32, False), ("mfma", 8, 8, True), ("mfma", 24, 32, False), ("mfma", 24, 5, True), ("mfma", 32, 1, False),
              ("valu", 12, 32, True), ("valu", 3, 7, False), ("valu", 32, 32, True), ("valu", 1, 1, False)]


def _conv_check(form, cin, cout, strided, m_dev=None):
    L, lib = _L()
    coords, feat, w, scale, shift, oc = vc.conv_case(cin, cout, CONV_SITES, CONV_DIMS, 7 * cin + cout + strided, strided)
    ref = vc.conv_ref(coords, feat, w, scale, shift, oc, CONV_DIMS, strided)
    same32 = vc.conv_ref(coords, feat, w, scale, shift, oc, CONV_DIMS, strided, torch.float32)
    got = _run_conv(L, lib, form, coords, feat, w, scale, shift, oc, CONV_DIMS, strided, m_dev=m_dev)
    n = len(oc) if m_dev is None else m_dev
    assert len(oc) > 64 and np.isfinite(got[:n]).all() and np.isnan(got[n:]).all(), "rows past the device row count were written"
    lim = vc.bound(ref, same32)
    err = float(np.abs(got[:n] - ref[:n]).max())
    tag = "" if m_dev is None else f", device row count {m_dev} of {len(oc)}"
    WORST[form] = max(WORST.get(form, 0.0), err / lim)
    print(f"sparse convolution {form} cin {cin} cout {cout} {'strided' if strided else 'submanifold'}{tag}: error {err:.3e}, bound {lim:.3e}, "
          f"ratio {err / lim:.3f} (worst of the {form} form so far {WORST[form]:.3f})")
    assert err <= lim, (err, lim)
    assert (ref > 0).sum() >= 50


@pytest.mark.parametrize("form,cin,cout,strided", FORM_CASES)
def test_the_fp32_forms_at_the_widths_the_pyramid_never_uses(form, cin, cout, strided):
    _conv_check(form, cin, cout, strided)


@pytest.mark.parametrize("form,cin,cout,strided", [("valu", 12, 32, False), ("mfma", 24, 32, False), ("split", 32, 32, False), ("split", 16, 24, True)])
def test_rows_past_the_device_row_count_are_left_alone(form, cin, cout, strided):
    """m_dev below m_cap and no multiple of 32: the cut falls inside a tile; `out` starts as NaN and stays NaN past the count"""
    _, _, _, _, _, oc = vc.conv_case(cin, cout, CONV_SITES, CONV_DIMS, 7 * cin + cout + strided, strided)
    m_dev = len(oc) - 45 - (1 if (len(oc) - 45) % 32 == 0 else 0)
    assert 0 < m_dev < len(oc) and m_dev % 32 and (len(oc) - 1) // 32 > m_dev // 32
    _conv_check(form, cin, cout, strided, m_dev=m_dev)


@pytest.mark.parametrize("width", [32, 24])
def test_the_fused_volume_write_and_the_scatter_launch_give_the_same_volume(width):
    """A level whose last convolution is the split form (cin 32) writes its rows into the dense volume itself; any other width (24:
    the fp32 matrix form) takes the gpnerf_sparse_scatter_dense launch.  Both are the float64 dense pyramid, and the volume is the
    scatter of the level's rows by the public entry point."""
    L, lib = _L()
    vol = _vol()
    dims = (16, 32, 16)
    coords, _ = vc.crowded(51, dims, 450)
    net = vc.random_net(vol, 1, 16, [width], 200 + width)
    assert [vol.SparseConvNet._split16(net.net[2][3]), net.net[2][3].cin] == [width == 32, width]
    code = torch.randn((len(coords), 16), generator=torch.Generator().manual_seed(width))
    _levels_vs_float64(net, code, coords, dims, f"one-level net, last convolution cin {width}")
    # the level's rows: with one level the runner's last convolution writes the plan's first feature buffer (rows of 32 floats)
    net = net.to(DEV)
    coord4 = torch.cat([torch.zeros((len(coords), 1), dtype=torch.long), torch.from_numpy(coords).long()], 1).to(DEV)
    plan = net.plan_levels(coord4, list(dims))
    with torch.no_grad():
        level = net.dense_levels_hip(code.to(DEV), coord4, list(dims), plan=plan)[0]
    grid, d, oc, om, cap, _ = plan["levels"][0]
    n = int(om.cpu()[0])
    rows = plan["feat"][0].reshape(-1)[: n * width].reshape(n, width).contiguous()
    again = torch.full(tuple(d) + (width,), float("nan"), device=DEV)
    L.check(lib.gpnerf_sparse_scatter_dense(rows.data_ptr(), width, oc.data_ptr(), grid.data_ptr(), om.data_ptr(), cap, I3(*d), again.data_ptr(), 0, None),
            "scatter")
    torch.cuda.synchronize()
    assert n > 100 and torch.equal(again, level)


@pytest.mark.parametrize("owner", ["highest", "lowest"])
@pytest.mark.parametrize("channels", [32, 5])
def test_the_scatter_lands_the_owners_row_of_a_shared_voxel(crowd, channels, owner):
    """gpnerf_sparse_to_dense on rows that share voxels: the row the index grid names lands, the others do not, unvisited cells are 0.
    With gpnerf_sparse_index's grid the owner is the voxel's highest row, which a scatter WITHOUT the owner test would tend to write
    last anyway; a grid that names the LOWEST row (the grid is an argument like any other) takes that luck away."""
    dims, coords, _, comp = crowd
    L, lib = _L()
    m = len(coords)
    feat = np.random.default_rng(channels).standard_normal((m, channels)).astype(np.float32)
    cd, grid = _index(L, lib, coords, dims)
    g = vc.index_grid(coords, dims)
    assert np.array_equal(grid.cpu().numpy(), g)
    if owner == "lowest":
        for o, others in comp.items():
            g[tuple(coords[o])] = others[0]
        grid = _t(g.astype(np.int32))
    fd = _t(feat)
    vol = torch.full(dims + (channels,), float("nan"), device=DEV)
    L.check(lib.gpnerf_sparse_to_dense(fd.data_ptr(), channels, cd.data_ptr(), grid.data_ptr(), None, m, I3(*dims), vol.data_ptr(), None), "to_dense")
    torch.cuda.synchronize()
    want = np.where((g >= 0)[..., None], feat[np.maximum(g, 0)], np.float32(0))
    assert np.array_equal(vol.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- 5. the host caches ----------------------------------------------------------------------------------------------------------------
def _cache_case(in_dim, width, seed, randomise_bn=True):
    dims = (16, 32, 16)
    coords, _ = vc.crowded(seed, dims, 450)
    coord4 = torch.cat([torch.zeros((len(coords), 1), dtype=torch.long), torch.from_numpy(coords).long()], 1).to(DEV)
    code = torch.randn((len(coords), in_dim), generator=torch.Generator().manual_seed(seed)).to(DEV)
    net = vc.random_net(_vol(), 1, in_dim, [width], seed, randomise_bn).to(DEV)

    def run(n):
        with torch.no_grad():
            return n.dense_levels_hip(code, coord4, list(dims))[0].clone()

    def fresh(n):
        """a net built from scratch that carries n's parameters: no cache of n's can reach it"""
        f = _vol().SparseConvNet(n_layers=1, in_dim=in_dim, out_dim=[width]).eval()
        f.load_state_dict({k: v.detach().cpu().clone() for k, v in n.state_dict().items()}, strict=True)
        return run(f.to(DEV))

    return net, run, fresh


def _same_as_fresh(net, run, fresh, before, what):
    got, want = run(net), fresh(net)
    assert not torch.equal(want, before), f"{what}: the change does not reach the volume, the case checks nothing"
    assert torch.equal(got, want), f"{what}: a stale cache served the last frame's values" if torch.equal(got, before) else what
    return got


def test_the_host_caches_follow_every_in_place_change():
    """_folded_bn, _packed_weight and _conv_table are keyed on data_ptr and _version: after each change the net must give, bit for bit,
    what a freshly built net with the same parameters gives."""
    # VALU form (cin 12: both vertex convolutions and the strided one), split form (32); then fp32 matrix form (24)
    for in_dim, width, convs in [(12, 32, {"valu": (0, 3), "valu strided": (1, 0), "split": (2, 3)}), (24, 24, {"mfma vertex": (0, 0), "mfma": (2, 0)})]:
        net, run, fresh = _cache_case(in_dim, width, 300 + in_dim)
        last = run(net)
        assert torch.equal(last, run(net)) and torch.equal(last, fresh(net))
        with torch.no_grad():
            for name, (block, at) in convs.items():
                net.net[block][at].weight.mul_(1.25)
                last = _same_as_fresh(net, run, fresh, last, f"{name} conv.weight.mul_")
            for block, at in [(0, 1), (2, 4)]:
                bn = net.net[block][at]
                bn.running_var.mul_(1.5)
                last = _same_as_fresh(net, run, fresh, last, "running_var")
                bn.weight.mul_(0.8)
                last = _same_as_fresh(net, run, fresh, last, "bn.weight")
                bn.bias.add_(0.05)
                last = _same_as_fresh(net, run, fresh, last, "bn.bias")
                bn.running_mean.add_(0.05)
                last = _same_as_fresh(net, run, fresh, last, "running_mean")
        other = vc.random_net(_vol(), 1, in_dim, [width], 999)
        net.load_state_dict(other.state_dict())
        last = _same_as_fresh(net, run, fresh, last, "load_state_dict")
        assert torch.equal(last, run(other.to(DEV)))
        net = net.cpu()
        with torch.no_grad():
            net.net[1][0].weight.mul_(0.9)                       # (changed while away, so that the round trip has something to show)
        net = net.to(DEV)
        last = _same_as_fresh(net, run, fresh, last, "cpu() and back")
        twin = copy.deepcopy(net)
        assert twin.__dict__.get("_conv_table_cache") is None    # _NotCopied: the copy builds its own table
        assert torch.equal(run(twin), last)
        with torch.no_grad():
            twin.net[2][0].weight.mul_(1.1)
        _same_as_fresh(twin, run, fresh, last, "deepcopy, then changed")
        assert torch.equal(run(net), last), "the copy's change reached the original"


@pytest.mark.parametrize("name", ["running_var", "running_mean", "weight", "bias"])
def test_the_host_caches_follow_a_rebound_batchnorm_tensor(name):
    """A buffer (or parameter) re-bound to a NEW tensor that has its predecessor's version -- `bn.running_var = torch.full_like(...)`
    on a net whose buffers were never modified: both have version 0 -- so only the pointer tells the two apart."""
    net, run, fresh = _cache_case(16, 32, 400, randomise_bn=False)
    bn = net.net[2][1]
    old = getattr(bn, name)
    before = run(net)
    new = torch.full_like(old.detach(), 2.0 if name in ("running_var", "weight") else 0.3)
    if name in ("weight", "bias"):
        new = torch.nn.Parameter(new)
    with torch.no_grad():
        while new._version < old._version:                       # (a parameter moved to the device arrives with version 1)
            new.add_(0)
    assert new._version == old._version and new.data_ptr() != old.data_ptr()
    if name == "running_var":
        assert old._version == 0
    setattr(bn, name, new)
    _same_as_fresh(net, run, fresh, before, f"bn.{name} re-bound")


# ---- 6. rows outside the grid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim", [16, 12])
def test_rows_outside_the_grid_are_ignored(in_dim):
    """Twelve rows with -1, dim or dim + 3 on one axis (the only values used: every access with them is range-checked or clamped)
    among the crowded rows: the levels are, bit for bit, those of the list without them -- removal keeps the other rows' order, so
    the ordered merges are the same sums.  A -1 row must not mark coarse site 0 of its axis (it would hold max(bn_shift, 0))."""
    dims = (16, 32, 16)
    coords, _ = vc.crowded(61, dims, 450)
    rows, keep = vc.outside_rows(coords, dims, 2)
    net = vc.random_net(_vol(), 2, in_dim, [32, 32], 500 + in_dim).to(DEV)
    code = torch.randn((len(rows), in_dim), generator=torch.Generator().manual_seed(6))

    def run(c, f):
        coord4 = torch.cat([torch.zeros((len(c), 1), dtype=torch.long), torch.from_numpy(c).long()], 1).to(DEV)
        with torch.no_grad():
            return [v.clone() for v in net.dense_levels_hip(f.to(DEV), coord4, list(dims))]

    clean = run(coords, code[torch.from_numpy(keep)])
    dirty = run(rows, code)
    for lv, (a, b) in enumerate(zip(dirty, clean)):
        extra = int(((a != 0).any(-1) & ~(b != 0).any(-1)).sum())
        assert extra == 0, f"level {lv + 1}: {extra} sites that only a row outside the grid reaches"
        assert torch.equal(a, b), lv
