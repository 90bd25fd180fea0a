#!/usr/bin/env python3
"""Generate the visual-hull vectors tests/golden/hull/*.npz by RUNNING the reference's ZjumocapDataset.prepare_inside_pts
(libs/datasets/ZjumocapDataset.py:259-283, with data_utils.project) on lattices from frame.dataset_lattice_axes.

    python tests/golden/make_golden_hull.py /path/to/GP-NeRF

The function is called unbound, with a stand-in `self` that carries `inside_view` and a `get_mask` returning the case's masks; the
reference is imported at run time behind inert stand-ins for the packages its dataset module imports and this machine may lack (cv2,
imageio, trimesh, torchvision, termcolor, yacs, PIL) -- none of them is touched by the two functions that run.  This file holds
none of the reference's text.

Every case stores its inputs (axes, masks, cams = K | RT with T in metres, exactly the array the reference builds at :268), the
reference's `inside`, a SHA-256 of the inputs and the number of near-tie points (tests/hull_cases.py: a projected coordinate within
1e-9 px of k + 0.5 in a view that tests the point).  The generator asserts what each case is there to show, and that the reference's
output equals the numpy restatement outside the near-tie points."""
import importlib
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import hull_cases as hc  # noqa: E402

STAND_INS = ("cv2", "imageio", "trimesh", "torchvision", "termcolor", "yacs", "PIL")


class _Inert(types.ModuleType):
    """a package-like module whose every attribute is an inert class"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


class _InertFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def __init__(self, names):
        self.names = names

    def find_spec(self, fullname, path, target=None):
        if fullname.split(".")[0] in self.names:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Inert(spec.name)

    def exec_module(self, module):
        pass


def reference_function(ref_root):
    missing = []
    for n in STAND_INS:
        try:
            importlib.import_module(n)
        except Exception:
            missing.append(n)
    sys.meta_path.append(_InertFinder(tuple(missing)))
    sys.path.insert(0, ref_root)
    return importlib.import_module("libs.datasets.ZjumocapDataset").ZjumocapDataset.prepare_inside_pts


def look_at(eye, target, up, roll=0.0):
    """world -> camera rotation (rows x, y, z of the camera) and T in metres"""
    z = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    R = np.stack([c * x + s * y, -s * x + c * y, z])
    return R, -R @ np.asarray(eye, np.float64)


def blob_mask(h, w, cy, cx, ry, rx, band):
    """1 inside an ellipse, 100 on a band around it (get_mask's erode / dilate border, :68-86), 0 outside"""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    m = np.zeros((h, w), np.uint8)
    m[((yy - cy) / (ry + band)) ** 2 + ((xx - cx) / (rx + band)) ** 2 <= 1.0] = 100
    m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 1
    return m


def box(centre, half):
    c, h = np.asarray(centre, np.float32), np.asarray(half, np.float32)
    return np.stack([c - h, c + h]).astype(np.float32)


def ring_cameras(rng, n, centre, dist, focal, h, w):
    Ks, Rs, Ts = [], [], []
    for i in range(n):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        R, T = look_at(centre + dist * d, centre + rng.normal(scale=0.01, size=3), rng.normal(size=3), roll=rng.uniform(-0.4, 0.4))
        Ks.append(np.array([[focal * rng.uniform(0.95, 1.05), 0.0, (w - 1) / 2 + rng.uniform(-3, 3)],
                            [0.0, focal * rng.uniform(0.95, 1.05), (h - 1) / 2 + rng.uniform(-3, 3)], [0.0, 0.0, 1.0]]))
        Rs.append(R)
        Ts.append(T)
    return Ks, Rs, Ts


def case_body(F):
    rng = np.random.default_rng(101)
    centre = np.array([0.0137, -0.0211, 0.0093])
    axes = F.dataset_lattice_axes(box(centre, (0.14, 0.22, 0.07)), (0.005, 0.005, 0.005))
    h, w = 96, 128
    Ks, Rs, Ts = ring_cameras(rng, 4, centre, 1.0, 520.0, h, w)
    masks = np.stack([blob_mask(h, w, 47 + 3 * i, 63 - 4 * i, 34 + 2 * i, 50 - 3 * i, 6) for i in range(4)])
    return axes, masks, Ks, Rs, Ts


def case_one(F):
    rng = np.random.default_rng(102)
    centre = np.array([-0.0071, 0.0113, 0.4021])
    axes = F.dataset_lattice_axes(box(centre, (0.05, 0.07, 0.04)), (0.005, 0.005, 0.005))
    h, w = 64, 80
    Ks, Rs, Ts = ring_cameras(rng, 1, centre, 0.8, 300.0, h, w)
    return axes, blob_mask(h, w, 30, 41, 14, 19, 4)[None], Ks, Rs, Ts


def case_close(F):
    """view 0: the camera's centre is a lattice point's z-plane inside the box, the optical axis along +z (rolled about it, so the
    image axes are in general position): the points below the plane are behind the camera, the plane itself has h2 == 0 exactly"""
    rng = np.random.default_rng(103)
    centre = np.array([0.0113, 0.0171, -0.0083])
    axes = F.dataset_lattice_axes(box(centre, (0.06, 0.06, 0.06)), (0.005, 0.005, 0.005))
    h, w = 72, 88
    k0 = 9
    eye = np.array([centre[0] + 0.0119, centre[1] - 0.0077, np.float64(axes[2][k0])])
    a = 0.37
    R0 = np.array([[np.cos(a), np.sin(a), 0.0], [-np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    T0 = -R0 @ eye
    T0[2] = -np.float64(axes[2][k0])                       # c2 = p2 * 1 + T3 is exactly 0 on the plane k0
    K0 = np.array([[61.3, 0.0, 43.1], [0.0, 59.7, 35.6], [0.0, 0.0, 1.0]])
    Ks, Rs, Ts = ring_cameras(rng, 2, centre, 0.7, 330.0, h, w)
    masks = np.stack([blob_mask(h, w, 35, 43, 22, 28, 5), blob_mask(h, w, 36, 44, 20, 26, 5), blob_mask(h, w, 34, 42, 21, 27, 5)])
    masks[0, :4, :4] = 1                                   # what INT32_MIN clips to; the other three corners stay 0
    return axes, masks, [K0] + Ks, [R0] + Rs, [T0] + Ts


def case_eight(F):
    rng = np.random.default_rng(104)
    centre = np.array([0.0031, -0.0057, 0.0119])
    axes = F.dataset_lattice_axes(box(centre, (0.0044, 0.0094, 0.3219)), (0.005, 0.005, 0.005))
    assert tuple(len(a) for a in axes) == (3, 5, 130), [len(a) for a in axes]
    h, w = 96, 128
    Ks, Rs, Ts = ring_cameras(rng, 8, centre, 1.5, 150.0, h, w)
    masks = np.stack([blob_mask(h, w, 47 + (i % 3), 63 - (i % 4), 24 - 9 * (i == 7), 31 - 12 * (i == 7), 4) for i in range(8)])
    return axes, masks, Ks, Rs, Ts


def millimetres(t):
    """T as the dataset's annotations hold it (mm), chosen where possible so that the reference's `/ 1000.` gives back exactly t
    (metres); hull_close's exact camera plane needs that, and asserts it"""
    out = []
    for v in np.asarray(t, np.float64).ravel():
        m = v * 1000.0
        for _ in range(8):
            if m / 1000.0 == v:
                break
            m = np.nextafter(m, np.inf if m / 1000.0 < v else -np.inf)
        out.append([float(m)])
    return out


def per_view(axes, masks, cams):
    """every point against every view on its own: (value [n,P], x [n,P], y [n,P])"""
    p = hc.lattice_points(axes).astype(np.float64)
    n, mh, mw = masks.shape
    V, X, Y = [], [], []
    for w_ in range(n):
        x, y = hc.project_view(p, cams[w_])
        col, _ = hc.pixel_of(x, mw - 1)
        row, _ = hc.pixel_of(y, mh - 1)
        V.append(masks[w_][row, col])
        X.append(x)
        Y.append(y)
    return np.stack(V), np.stack(X), np.stack(Y)


def main(ref_root):
    F = importlib.import_module("gp-nerf_amd.frame")
    fn = reference_function(ref_root)
    out_dir = os.path.join(HERE, "hull")
    os.makedirs(out_dir, exist_ok=True)
    for name, make in (("hull_body", case_body), ("hull_one", case_one), ("hull_close", case_close), ("hull_eight", case_eight)):
        axes, masks, Ks, Rs, Ts = make(F)
        n = len(Ks)
        # the reference's own inputs: T in millimetres, a column; RT is built from them exactly as :268 does
        cam_dict = {"K": [k.tolist() for k in Ks], "R": [r.tolist() for r in Rs], "T": [millimetres(t) for t in Ts]}
        RTs = [np.concatenate([np.array(cam_dict["R"][v]), np.array(cam_dict["T"][v]) / 1000.], axis=1) for v in range(n)]
        cams = hc.cams_of([np.array(k) for k in cam_dict["K"]], RTs)
        pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).astype(np.float32)
        stub = types.SimpleNamespace(inside_view=list(range(n)), get_mask=lambda seq, img: masks[img])
        with np.errstate(all="ignore"):
            inside = fn(stub, pts, 0, cam_dict, list(range(n)), None)
        assert inside.dtype == np.uint8 and inside.shape == pts.shape[:3]
        ref, tie, converted = hc.hull_np(axes, masks, cams)
        left_out = hc.compare_outside_ties(ref, inside, tie)
        V, X, Y = per_view(axes, masks, cams)
        mh, mw = masks.shape[1:]
        if name == "hull_body":
            assert ((V[0] == 100) & ((V[1:] == 0).any(0))).any(), "a band point of view 0 that a later view would have carved"
            assert ((V[0] == 0) & (V[1:] == 1).all(0)).any(), "a point only view 0 carves"
            tested = np.cumprod(np.concatenate([np.ones((1, V.shape[1]), bool), V[:-1] == 1]), axis=0).astype(bool)
            for side, hit in (("left", X < -0.5), ("right", X > mw - 0.5), ("top", Y < -0.5), ("bottom", Y > mh - 0.5)):
                assert (hit & tested).any(), f"no tested point projects outside the image on the {side}"
            assert set(np.unique(inside)) == {0, 1, 100}
        if name == "hull_close":
            p = hc.lattice_points(axes).astype(np.float64)
            RT0 = cams[0, 9:].reshape(3, 4)
            c2 = ((p[:, 0] * RT0[2, 0] + p[:, 1] * RT0[2, 1]) + p[:, 2] * RT0[2, 2]) + RT0[2, 3]
            eye = -RT0[:, :3].T @ RT0[:, 3]
            assert all(axes[a][0] < eye[a] < axes[a][-1] for a in range(3)), "the camera centre lies inside the lattice box"
            assert (c2 < 0).any() and (c2 == 0).any() and (c2 > 0).any()
            assert converted > 0, "no out-of-range / non-finite conversion"
        if name == "hull_eight":
            assert (V[:7] == 1).all(0).any(), "no point reaches the eighth view"
            assert set(np.unique(inside)) == {0, 1, 100} and len(set(np.unique(V[7][(V[:7] == 1).all(0)]))) > 1, "the eighth view carves"
        meta = {"case": name, "n_views": n, "dims": [len(a) for a in axes], "near_ties": left_out, "converted": converted,
                "counts": {str(int(v)): int(c) for v, c in zip(*np.unique(inside, return_counts=True))},
                "sha256_inputs": hc.sha_hull_inputs(axes, masks, cams), "numpy": np.__version__}
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), axis_x=axes[0], axis_y=axes[1], axis_z=axes[2], masks=masks, cams=cams,
                            inside=inside, meta_json=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
        print(name, meta)


if __name__ == "__main__":
    main(sys.argv[1])
