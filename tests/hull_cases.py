"""The visual hull of the dense renderer's geometry mode (ZjumocapDataset.prepare_inside_pts + data_utils.project) restated in numpy,
and the fixtures tests/golden/hull/*.npz (tests/golden/make_golden_hull.py: the reference's own function run on the same inputs).

The restatement is gpnerf_visual_hull's specification (include/gpnerf_hip.h): float64, multiply then add in source order (numpy's
elementwise operators do not fuse), rint (half to even), the out-of-range conversion to INT32_MIN made explicit, values not
booleans, a view tests only the points whose value is still exactly 1."""
import glob
import hashlib
import json
import os

import numpy as np

HULL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hull")
TIE_EPS = 1e-9            # px: a projected coordinate this close to k + 0.5 may round either way under another operation order
TIE_CAP = 1e-4            # at most this share of a case's points may be left out for it


def hull_case_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HULL_DIR, "*.npz")))


def load_hull(name):
    z = np.load(os.path.join(HULL_DIR, name + ".npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    axes = [np.ascontiguousarray(z[k], dtype=np.float32) for k in ("axis_x", "axis_y", "axis_z")]
    assert sha_hull_inputs(axes, z["masks"], z["cams"]) == meta["sha256_inputs"]
    return z, meta, axes


def sha_hull_inputs(axes, masks, cams):
    h = hashlib.sha256()
    for a in list(axes) + [masks, cams]:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def cams_of(Ks, RTs):
    """[n,3,3], [n,3,4] -> the entry point's [n,21] float64"""
    return np.ascontiguousarray(np.concatenate([np.asarray(Ks, np.float64).reshape(-1, 9), np.asarray(RTs, np.float64).reshape(-1, 12)], axis=1))


def project_view(p, cam):
    """p [P,3] float64, cam [21] -> (x, y) float64: data_utils.project (:246-249) written out"""
    K, RT = cam[:9].reshape(3, 3), cam[9:].reshape(3, 4)
    with np.errstate(all="ignore"):
        c = [((p[:, 0] * RT[r, 0] + p[:, 1] * RT[r, 1]) + p[:, 2] * RT[r, 2]) + RT[r, 3] for r in range(3)]
        h = [(c[0] * K[r, 0] + c[1] * K[r, 1]) + c[2] * K[r, 2] for r in range(3)]
        return h[0] / h[2], h[1] / h[2]


def pixel_of(v, hi):
    """np.clip(np.round(v).astype(np.int32), 0, hi) with x86-64's conversion: what is not finite or does not fit becomes INT32_MIN -> 0"""
    with np.errstate(all="ignore"):
        r = np.rint(v)
        bad = ~(np.abs(r) < 2147483648.0)
        q = np.where(bad, 0.0, r).astype(np.int64)
    return np.where(bad, 0, np.clip(q, 0, hi)), bad


def near_tie(v):
    with np.errstate(all="ignore"):
        return np.isfinite(v) & (np.abs((v - np.floor(v)) - 0.5) <= TIE_EPS)


def lattice_points(axes):
    """[P,3] float32, meshgrid 'ij' (x slowest): batch['pts'] flattened"""
    return np.stack(np.meshgrid(*[np.asarray(a, np.float32) for a in axes], indexing="ij"), axis=-1).reshape(-1, 3)


def hull_np(axes, masks, cams):
    """-> (inside uint8 [X,Y,Z], tie bool [X,Y,Z] = a view that tested the point projected it within TIE_EPS of a half pixel,
    converted int64 = conversions that went out of range in a view that tested the point)"""
    masks = np.asarray(masks, dtype=np.uint8)
    n, mh, mw = masks.shape
    p = lattice_points(axes).astype(np.float64)
    value = np.ones(len(p), dtype=np.uint8)
    tie = np.zeros(len(p), dtype=bool)
    converted = 0
    for w in range(n):
        ind = np.nonzero(value == 1)[0]
        if not len(ind):
            break
        x, y = project_view(p[ind], np.asarray(cams, np.float64).reshape(n, 21)[w])
        col, bx = pixel_of(x, mw - 1)
        row, by = pixel_of(y, mh - 1)
        converted += int(bx.sum() + by.sum())
        tie[ind] |= near_tie(x) | near_tie(y)
        value[ind] = masks[w][row, col]
    sh = tuple(len(a) for a in axes)
    return value.reshape(sh), tie.reshape(sh), converted


def compare_outside_ties(got, ref, tie):
    """got == ref except at near-tie points, which are at most TIE_CAP of the case's points; returns the number left out"""
    assert got.shape == ref.shape and got.dtype == np.uint8
    left_out = int(tie.sum())
    assert left_out <= TIE_CAP * tie.size, (left_out, tie.size)
    bad = (got != ref) & ~tie
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    return left_out
