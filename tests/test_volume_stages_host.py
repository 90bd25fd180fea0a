"""CPU: the cases and restatements of tests/volume_cases.py, which tests/test_gpu_volume_stages.py holds the sparse volume builder's
kernels to stage by stage -- that the crowded case is as crowded as it claims, that the restatements agree with
oracle/producers_ref.py and with float64, and that the rows outside the grid would matter if they were not ignored."""
import importlib

import numpy as np
import pytest
import torch

import volume_cases as vc
from oracle import producers_ref as pref


@pytest.mark.parametrize("dims,singles", [((8, 16, 8), 150), ((16, 32, 16), 450)])
def test_the_crowded_case_holds_the_multiplicities_it_is_for(dims, singles):
    coords, planted = vc.crowded(3, dims, singles)
    assert len(coords) == 375 + singles and len(coords) % 64 != 0
    assert vc.in_grid(coords, dims).all()
    cells, counts = np.unique(coords, axis=0, return_counts=True)
    got = {tuple(int(v) for v in c): int(n) for c, n in zip(cells, counts)}
    assert sorted(planted.values()) == sorted(vc.PLANTED) == sorted(n for n in got.values() if n > 1)
    assert all(got[c] == n for c, n in planted.items()) and sum(n == 1 for n in got.values()) == singles
    # 9 rows fill the owner's slots, 10 are the first to scan
    assert 9 - 1 == vc.DUP_SLOTS and 10 - 1 > vc.DUP_SLOTS
    grid, comp = vc.index_grid(coords, dims), vc.companions(coords, dims)
    assert len(comp) == len(planted)
    for cell, n in planted.items():
        rows = np.nonzero((coords == np.array(cell)).all(1))[0]
        owner = int(grid[cell])
        assert owner == rows.max() and comp[owner] == sorted(rows[:-1].tolist()) and len(rows) == n
        if n > 64:
            # the rows of a scanned voxel are spread over the list: several 64-row chunks, and the owner is not the list's last row
            assert len(set(rows // 64)) >= 4 and owner != len(coords) - 1
    # face, edge and corner neighbours among the planted voxels, and planted voxels on the border
    pc = np.array(list(planted))
    steps = {int(np.abs(a - b).sum()) for a in pc for b in pc if np.abs(a - b).max() == 1}
    assert steps == {1, 2, 3}
    assert any((np.array(c) == 0).any() for c in planted) and any((np.array(c) == np.array(dims) - 1).any() for c in planted)
    again, _ = vc.crowded(3, dims, singles)
    other, _ = vc.crowded(4, dims, singles)
    assert np.array_equal(coords, again) and not np.array_equal(coords, other)


def test_the_index_restatement_is_the_oracles_lookup():
    dims = (8, 16, 8)
    coords, _ = vc.crowded(5)
    x = pref.SparseTensor(torch.zeros(len(coords), 1), torch.from_numpy(coords).long(), dims)
    sk, order = torch.sort(x.keys(), stable=True)
    cells = torch.arange(int(np.prod(dims)))
    assert np.array_equal(pref._lookup(sk, order, cells).numpy(), vc.index_grid(coords, dims).reshape(-1))


@pytest.mark.parametrize("channels", [32, 5])
def test_the_ordered_merge_is_the_float64_sum_within_float32_rounding(channels):
    dims = (8, 16, 8)
    coords, planted = vc.crowded(7)
    feat = np.random.default_rng(channels).standard_normal((len(coords), channels)).astype(np.float32)
    got, count = vc.merge_ordered(feat, coords, dims)
    exact = vc.merge_exact(feat, coords, dims)
    comp = vc.companions(coords, dims)
    owners = sorted(comp)
    assert got.dtype == np.float32 and sorted(count[owners] + 1) == sorted(vc.PLANTED) and count.sum() == 375 - len(planted)
    rest = np.setdiff1d(np.arange(len(coords)), owners)
    assert np.array_equal(got[rest], feat[rest]) and np.array_equal(exact[rest], feat[rest].astype(np.float64))
    for o in owners:
        # n additions, each within half an ulp of a partial sum that the sum of magnitudes bounds
        n = int(count[o])
        limit = n * 2.0 ** -24 * np.abs(feat[[o] + comp[o]].astype(np.float64)).sum(0)
        assert np.all(np.abs(got[o] - exact[o]) <= limit), (o, n)
    assert np.abs(got[owners] - exact[owners]).max() > 0          # float32 did round: the order is something to get right
    # the order matters to the bits: the same rows added highest first give other words somewhere
    o = max(owners, key=lambda r: count[r])
    acc = feat[o].copy()
    for r in reversed(comp[o]):
        acc = (acc + feat[r]).astype(np.float32)
    assert not np.array_equal(acc, got[o])


@pytest.mark.parametrize("out_dims,m", [((8, 16, 8), 256), ((16, 40, 24), 2500), ((9, 25, 11), 600)])
def test_the_reachable_sites_are_the_oracles_strided_sites(out_dims, m):
    in_dims = tuple(2 * n for n in out_dims)
    g = np.random.default_rng(m)
    coords = np.stack([g.integers(0, n, m) for n in in_dims], 1).astype(np.int32)            # with repeats
    want = vc.reachable_sites(coords, out_dims)
    y = pref.sparse_conv3d(pref.SparseTensor(torch.zeros(m, 1), torch.from_numpy(coords).long(), in_dims), torch.zeros(3, 3, 3, 1, 1), 2, 1)
    assert y.shape == out_dims
    assert {tuple(r) for r in y.coords.tolist()} == {tuple(r) for r in want.tolist()} and len(want) == y.coords.shape[0]
    assert 0 < len(want) < int(np.prod(out_dims))                 # some sites stay unreached: "every other cell is -1" says something
    # a fine site reaches between 1 and 8 coarse sites
    one = vc.reachable_sites(np.array([[2, 2, 2]]), out_dims)
    eight = vc.reachable_sites(np.array([[3, 3, 3]]), out_dims)
    assert one.tolist() == [[1, 1, 1]] and len(eight) == 8


def test_the_conv_restatement_is_the_oracles_and_float32_is_close():
    dims = (8, 16, 8)
    for strided in (False, True):
        coords, feat, w, scale, shift, oc = vc.conv_case(8, 5, 300, dims, 11 + strided, strided)
        ref = vc.conv_ref(coords, feat, w, scale, shift, oc, dims, strided)
        x = pref.SparseTensor(torch.from_numpy(feat).double(), torch.from_numpy(coords).long(), dims)
        wt = torch.from_numpy(w).double().view(3, 3, 3, 8, 5)
        y = pref.sparse_conv3d(x, wt, 2, 1) if strided else pref.sparse_conv3d(x, wt, subm=True)
        dense = torch.relu(y.features * torch.from_numpy(scale).double() + torch.from_numpy(shift).double())
        key = {tuple(c): i for i, c in enumerate(y.coords.tolist())}
        rows = [key[tuple(c)] for c in oc.tolist()]
        assert np.abs(dense[rows].numpy() - ref).max() < 1e-12
        same32 = vc.conv_ref(coords, feat, w, scale, shift, oc, dims, strided, torch.float32)
        assert same32.dtype == np.float32 and 0 < np.abs(same32 - ref).max() < 1e-5
        assert 2.0 ** -22 <= vc.bound(ref, same32) < 1e-4


def test_rows_outside_the_grid_would_matter_if_they_were_not_ignored():
    dims = (16, 32, 16)
    coords, _ = vc.crowded(9, dims, 450)
    rows, keep = vc.outside_rows(coords, dims, 1)
    assert np.array_equal(rows[keep], coords) and (~keep).sum() == 12
    extra = rows[~keep]
    bad = ~((extra >= 0) & (extra < np.array(dims)))
    assert (bad.sum(1) == 1).all() and bad.any(0).all()
    assert sorted(set(extra[bad].tolist()) - {-1}) == sorted({d for d in dims} | {d + 3 for d in dims})
    assert not vc.in_grid(extra, dims).any()
    out_dims = tuple(d // 2 for d in dims)
    clean = {tuple(s) for s in vc.reachable_sites(coords, out_dims).tolist()}
    assert {tuple(s) for s in vc.reachable_sites(rows, out_dims).tolist()} == clean
    phantom = {tuple(s) for s in vc.reachable_sites(rows, out_dims, skip_negative=False).tolist()} - clean
    assert phantom and all(0 in s for s in phantom)               # only the -1 rows reach anything, and only site 0 of their axis
    # the index and the merge ignore them too: the same grid up to the rows' renumbering
    g_all, g_clean = vc.index_grid(rows, dims), vc.index_grid(coords, dims)
    renumber = np.cumsum(keep) - 1
    assert np.array_equal(np.where(g_all >= 0, renumber[np.maximum(g_all, 0)], -1), g_clean)


def test_the_stage_entry_points_check_their_arguments():
    L = importlib.import_module("gp-nerf_amd._lib")
    lib = L.lib()
    import ctypes as C
    I3 = C.c_int32 * 3
    p = 0x1000
    assert lib.gpnerf_sparse_merge_duplicates(p, 33, p, p, 8, I3(8, 8, 8), p, None) == -1           # more than 32 channels
    assert lib.gpnerf_sparse_merge_duplicates(p, 32, p, p, 0, I3(8, 8, 8), p, None) == 0            # nothing to do
    assert lib.gpnerf_sparse_down_sites(p, None, 8, I3(8, 0, 8), p, p, p, 8, None) == -1
    assert lib.gpnerf_sparse_conv3_mfma(0, p, 12, p, I3(8, 8, 8), p, None, 8, p, 8, p, p, p, None) == -1   # cin no multiple of 8
    assert lib.gpnerf_sparse_conv3(0, p, 12, p, I3(8, 8, 8), p, None, 8, p, 33, p, p, p, None) == -1       # cout > 32
    assert lib.gpnerf_sparse_to_dense(p, 40, p, p, None, 8, I3(8, 8, 8), p, None) == -1
    assert lib.gpnerf_sparse_packed_weight_floats(24) == 27 * 3 * 256 and lib.gpnerf_sparse_packed_weight_floats(12) == 0
