"""Cases and float64 / ordered-float32 restatements for the stages of the sparse volume builder (csrc/gpnerf_volume.hip), one stage
at a time: the index grid, the ordered merge of rows that share a voxel, the coarse sites of a strided convolution, the convolution
forms with BatchNorm + ReLU, the scatter.  No GPU code: tests/test_volume_stages_host.py pins what is here on the CPU,
tests/test_gpu_volume_stages.py holds the kernels to it."""
import numpy as np
import torch

DUP_SLOTS = 8                                              # csrc/gpnerf_volume.hip: companions an owner finds without scanning
PLANTED = (2, 8, 9, 10, 11, 64, 65, 66, 140)               # rows per planted voxel: 9 fills the slots, 10 is the first scan, 65 / 66
                                                           # straddle a 64-row scan chunk


def _planted_cells(dims):
    """multiplicity -> cell.  (9, 10, 65) are face / corner / edge neighbours of each other, (2, 8) face neighbours; 140 sits in the
    grid's first corner and 66 in its last."""
    D, H, W = dims
    return {140: (0, 0, 0), 66: (D - 1, H - 1, W - 1), 9: (3, 5, 3), 10: (3, 5, 4), 65: (4, 6, 4), 2: (5, 10, 2), 8: (5, 11, 2),
            11: (1, 8, 6), 64: (6, 3, 5)}


def crowded(seed, dims=(8, 16, 8), singles=150):
    """A shuffled row list whose voxels are crowded on purpose: coords int32 [m, 3] and {cell: rows in it} of the planted voxels.
    m = 375 + singles (525: no multiple of 64)."""
    g = np.random.default_rng(seed)
    planted = {cell: n for n, cell in _planted_cells(dims).items()}
    taken = {np.ravel_multi_index(c, dims) for c in planted}
    free = np.array([i for i in range(int(np.prod(dims))) if i not in taken])
    lone = np.stack(np.unravel_index(g.choice(free, size=singles, replace=False), dims), 1)
    rows = [np.repeat(np.array([c]), n, axis=0) for c, n in planted.items()] + [lone]
    coords = np.concatenate(rows).astype(np.int32)
    order = g.permutation(len(coords))
    last = int(np.nonzero(order >= 375)[0][-1])             # the list ends in a single-row voxel: no planted voxel's owner is the last row
    order[[last, -1]] = order[[-1, last]]
    return np.ascontiguousarray(coords[order]), planted


def in_grid(coords, dims):
    return np.all((coords >= 0) & (coords < np.array(dims)), axis=1)


def index_grid(coords, dims):
    """cell -> the HIGHEST row in it (-1: none); a row with a coordinate outside the grid is ignored (index_kernel)."""
    grid = -np.ones(dims, np.int64)
    for r in np.nonzero(in_grid(coords, dims))[0]:          # ascending: the highest row stays
        grid[tuple(coords[r])] = r
    return grid


def companions(coords, dims):
    """{owner row: the other rows of its voxel, ascending} for every voxel that holds more than one row."""
    grid = index_grid(coords, dims)
    out = {}
    for r in np.nonzero(in_grid(coords, dims))[0]:
        o = int(grid[tuple(coords[r])])
        if o != r:
            out.setdefault(o, []).append(int(r))
    return out


def merge_ordered(feat, coords, dims):
    """gpnerf_sparse_merge_duplicates in its documented order, reproducible in float32: the owner's value first, then the other rows
    of the voxel in ascending row order.  Returns (merged [m, c] float32, count [m])."""
    out = feat.astype(np.float32).copy()
    count = np.zeros(len(feat), np.int32)
    for o, others in companions(coords, dims).items():
        acc = feat[o].astype(np.float32)
        for r in others:
            acc = (acc + feat[r].astype(np.float32)).astype(np.float32)
        out[o], count[o] = acc, len(others)
    return out, count


def merge_exact(feat, coords, dims):
    """the same sums in float64 (no order to speak of)"""
    out = feat.astype(np.float64).copy()
    for o, others in companions(coords, dims).items():
        out[o] = feat[[o] + others].astype(np.float64).sum(0)
    return out


def reachable_sites(coords, out_dims, skip_negative=True):
    """Every coarse site some tap of some row reaches under k3 s2 p1 (site o reads the positions 2 o - 1 + k): an int64 [n, 3] array,
    sorted by cell.  skip_negative: a row with a negative coordinate is outside the grid and ignored, which is the builder's contract;
    False restates the arithmetic alone, under which p = -1 reaches site 0 through tap 0."""
    sites = set()
    for p in np.asarray(coords, np.int64):
        if skip_negative and (p < 0).any():
            continue
        per_axis = []
        for a in range(3):
            per_axis.append([(p[a] + 1 - k) // 2 for k in range(3) if (p[a] + 1 - k) >= 0 and (p[a] + 1 - k) % 2 == 0 and (p[a] + 1 - k) // 2 < out_dims[a]])
        sites.update((d, h, w) for d in per_axis[0] for h in per_axis[1] for w in per_axis[2])
    return np.array(sorted(sites), np.int64).reshape(-1, 3)


def conv_case(cin, cout, m, dims, seed, strided):
    """Random active sites (one row each), features, weights [27][cin][cout] and folded BatchNorm factors; the output sites are the
    input's for the submanifold form and a subset of the reachable coarse sites for the strided one."""
    g = np.random.default_rng(seed)
    cells = g.choice(dims[0] * dims[1] * dims[2], size=m, replace=False)
    coords = np.stack(np.unravel_index(cells, dims), 1).astype(np.int32)
    feat = g.standard_normal((m, cin)).astype(np.float32)
    w = (g.standard_normal((27, cin, cout)) * 0.1).astype(np.float32)
    scale = g.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = (g.standard_normal(cout) * 0.2).astype(np.float32)
    oc = np.unique(coords // 2, axis=0).astype(np.int32) if strided else coords
    return coords, feat, w, scale, shift, np.ascontiguousarray(oc)


def conv_ref(coords, feat, w, scale, shift, oc, dims, strided, dtype=torch.float64):
    """out[o] = relu(scale * sum_k in[s o - 1 + k] W[k] + shift) through the index grid (the highest row of a voxel answers), every
    operation in `dtype` on the CPU: float64 is the reference, float32 the yardstick for what float32 arithmetic costs."""
    grid = index_grid(coords, dims)
    f, wt = torch.from_numpy(feat).to(dtype), torch.from_numpy(w).to(dtype)
    out = torch.zeros((len(oc), w.shape[2]), dtype=dtype)
    for k in range(27):
        p = (2 * oc if strided else oc).astype(np.int64) - 1 + np.array([k // 9, (k // 3) % 3, k % 3])
        ok = np.all((p >= 0) & (p < np.array(dims)), 1)
        j = np.full(len(oc), -1)
        j[ok] = grid[p[ok, 0], p[ok, 1], p[ok, 2]]
        hit = torch.from_numpy(j >= 0)
        if hit.any():
            out[hit] += f[torch.from_numpy(j[j >= 0])] @ wt[k]
    return torch.relu(out * torch.from_numpy(scale).to(dtype) + torch.from_numpy(shift).to(dtype)).numpy()


def bound(ref64, same32):
    """What a float32 kernel may miss the float64 reference by: 4 x what the same formula in float32 on the CPU misses it by (the factor
    allows for another order of the same additions), and never less than 2^-22 of the output range."""
    top = max(1.0, float(np.abs(ref64).max()))
    return max(4.0 * float(np.abs(np.asarray(same32, np.float64) - ref64).max()), 2.0 ** -22 * top)


def outside_rows(coords, dims, seed, n=12):
    """`coords` with n rows added that lie outside the grid on ONE axis -- by -1, dim or dim + 3, the only values used -- at random
    places of the list.  Returns (all rows, keep: mask of the original rows).  The rows with -1 are placed where the unguarded
    arithmetic of reachable_sites would reach a coarse site that no real row reaches."""
    g = np.random.default_rng(seed)
    out_dims = tuple(d // 2 for d in dims)
    real = {tuple(s) for s in reachable_sites(coords, out_dims)}
    extra = []
    for i in range(n):
        a, kind = i % 3, (i // 3) % 3
        for _ in range(1000):
            p = np.array([g.integers(0, d) for d in dims])
            p[a] = (-1, dims[a], dims[a] + 3)[kind]
            if kind or any(tuple(s) not in real for s in reachable_sites(p[None], out_dims, skip_negative=False)):
                break
        else:
            raise AssertionError("no place left where a -1 row would reach a site of its own")
        extra.append(p)
    m = len(coords) + n
    at = np.sort(g.choice(m, size=n, replace=False))
    keep = np.ones(m, bool)
    keep[at] = False
    rows = np.empty((m, 3), np.int32)
    rows[keep], rows[at] = coords, np.array(extra, np.int32)
    return rows, keep


def random_net(vol, n_layers, in_dim, out_dim, seed, randomise_bn=True):
    """the product's SparseConvNet in eval mode with random BatchNorm statistics (fresh ones are the identity)"""
    torch.manual_seed(seed)
    net = vol.SparseConvNet(n_layers=n_layers, in_dim=in_dim, out_dim=list(out_dim)).eval()
    if randomise_bn:
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.2)
    return net
