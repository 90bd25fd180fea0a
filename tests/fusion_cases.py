"""Cases and the numpy restatement for the depth-fusion tests (gpnerf_fusion.hip; include/gpnerf_hip.h states THE DEFINITION restated
here, rule for rule, gpnerf_fusion_integrate).

`integrate(state, ...)` is the definition in float64, vectorised over the lattice points, one view at a time in ascending order, on a
state it continues; `finalise(state, band)` the value and the totals; `restate(...)` both on a fresh state, in chunks of views when
asked: what the kernels must give bit for bit.  Nothing here looks at what the kernels give.
"""
import functools

import numpy as np

import mesh_metric_cases as mc
import raycast_cases as rc
import texture_cases as tc
from mesh_metric_cases import f32

BEHIND, OUTSIDE, NODATA, EMPTY, HIDDEN, NEAR = range(6)
FATES = ("behind", "outside", "nodata", "empty", "hidden", "near")
TOTALS = ("seen", "surface", "interior", "unknown")
FLAG_HIDDEN, FLAG_NEAR = 1, 2


def lattice_points(lo, step, dims):
    """the lattice's points, float32 [nx ny nz, 3], z fastest: float32(lo + double(i) * step) per axis"""
    lo, step = np.asarray(lo, np.float64), np.asarray(step, np.float64)
    axes = [(lo[a] + np.arange(dims[a], dtype=np.float64) * step[a]).astype(np.float32) for a in range(3)]
    g = np.meshgrid(*axes, indexing="ij")
    return np.stack([x.ravel() for x in g], axis=1)


def new_state(dims):
    n = int(np.prod(dims))
    return {"sum": np.zeros(n, np.float64), "weight": np.zeros(n, np.float64), "flags": np.zeros(n, np.uint8)}


def integrate(state, depth, Ks, RTs, lo, step, dims, band, weights=None, z_near=1e-6, carve=True):
    """rules 1-7 and the accumulation for the views of one call -> (stats int64 [V,6], fate [n,V]); the state is continued in place"""
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    Ks, RTs = np.asarray(Ks, np.float64).reshape(-1, 3, 3), np.asarray(RTs, np.float64).reshape(-1, 3, 4)
    assert len(Ks) == V and len(RTs) == V
    p = lattice_points(lo, step, dims)
    n = len(p)
    b = np.float64(np.float32(band))
    fate = np.full((n, V), -1, np.int64)
    with np.errstate(all="ignore"):
        for v in range(V):
            x, y, z = tc.project(p, Ks[v], RTs[v])
            open_ = np.ones(n, bool)

            def rule(name, hit):
                fate[open_ & hit, v] = name
                return open_ & ~hit

            open_ = rule(BEHIND, ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z >= np.float64(z_near))))
            open_ = rule(OUTSIDE, ~((x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)))
            row = np.where(open_, np.rint(y), 0).astype(np.int64)               # rint: half to even
            col = np.where(open_, np.rint(x), 0).astype(np.int64)
            d = depth[v][row, col]
            w = np.ones(n, np.float32) if weights is None else np.asarray(weights, np.float32)[v][row, col]
            open_ = rule(NODATA, ~(d > 0) | ~np.isfinite(w) | ~(w > 0) | (np.isposinf(d) & (not carve)))
            background = np.isposinf(d)
            s = d.astype(np.float64) - z
            t = np.where(~background & (s < b), s, b)
            open_ = rule(EMPTY, background)
            open_ = rule(HIDDEN, s < -b)
            open_ = rule(EMPTY, s >= b)
            fate[open_, v] = NEAR
            add = (fate[:, v] == EMPTY) | (fate[:, v] == NEAR)
            w64 = w.astype(np.float64)
            state["sum"][add] = state["sum"][add] + w64[add] * t[add]
            state["weight"][add] = state["weight"][add] + w64[add]
            state["flags"][fate[:, v] == HIDDEN] |= np.uint8(FLAG_HIDDEN)
            state["flags"][fate[:, v] == NEAR] |= np.uint8(FLAG_NEAR)
    assert (fate >= 0).all()
    stats = np.stack([[int((fate[:, v] == k).sum()) for k in range(6)] for v in range(V)]).astype(np.int64)
    return stats, fate


def finalise(state, band):
    """-> (values float32 [n], totals int64 [4])"""
    band = np.float32(band)
    seen = state["weight"] > 0
    interior = ~seen & ((state["flags"] & FLAG_HIDDEN) != 0)
    with np.errstate(all="ignore"):
        mean = np.clip((state["sum"] / state["weight"]).astype(np.float32), -band, band)
    values = np.where(seen, mean, np.where(interior, -band, band)).astype(np.float32)
    totals = np.array([seen.sum(), ((state["flags"] & FLAG_NEAR) != 0).sum(), interior.sum(), (~seen & ~interior).sum()], np.int64)
    return values, totals


def restate(depth, Ks, RTs, lo, step, dims, band, weights=None, z_near=1e-6, carve=True, chunks=None):
    """a fresh state, the views integrated in the groups `chunks` names (default: all at once), finalised ->
    {"values" float32 [dims], "flags" uint8 [dims], "sum", "weight" float64 [dims], "stats" int64 [V,6] (the calls' rows stacked),
    "totals" int64 [4], "fate" [n,V]}"""
    depth = np.asarray(depth, np.float32)
    V = len(depth)
    chunks = chunks if chunks is not None else [range(V)]
    state = new_state(dims)
    stats, fate = [], []
    for ch in chunks:
        ch = list(ch)
        s, f = integrate(state, depth[ch], np.asarray(Ks)[ch], np.asarray(RTs)[ch], lo, step, dims, band,
                         None if weights is None else np.asarray(weights)[ch], z_near, carve)
        stats.append(s)
        fate.append(f)
    values, totals = finalise(state, band)
    d = tuple(dims)
    return {"values": values.reshape(d), "flags": state["flags"].reshape(d), "sum": state["sum"].reshape(d), "weight": state["weight"].reshape(d),
            "stats": np.concatenate(stats), "totals": totals, "fate": np.concatenate(fate, axis=1)}


# ---------------------------------------------------------------- cases

def sphere_depth(Ks, RTs, H, W, radius, centre=(0.0, 0.0, 0.0)):
    """the analytic CAMERA-Z depth maps of a sphere, float32 [V,H,W], +inf where the pixel's ray misses it: the ray through pixel
    (column i, row j) is eye + t R^T inv(K) (i, j, 1), whose camera-z component is 1, so t is camera z"""
    Ks, RTs = np.asarray(Ks, np.float64).reshape(-1, 3, 3), np.asarray(RTs, np.float64).reshape(-1, 3, 4)
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.full((len(Ks), H, W), np.inf, np.float32)
    for v, (K, RT) in enumerate(zip(Ks, RTs)):
        R, T = RT[:, :3], RT[:, 3]
        o = -R.T @ T - np.asarray(centre, np.float64)
        cam = np.linalg.solve(K, np.stack([col.ravel(), row.ravel(), np.ones(H * W)]))
        d = (R.T @ (cam / cam[2])).T
        a, b, c = (d * d).sum(axis=1), d @ o, o @ o - radius * radius
        disc = b * b - a * c
        with np.errstate(invalid="ignore"):
            t = (-b - np.sqrt(disc)) / a
        hit = (disc >= 0) & (t > 0)
        out[v] = np.where(hit, t, np.inf).reshape(H, W).astype(np.float32)
    return out


def axis_cameras(H, W, focal, distance):
    """six look_at cameras on +x, -x, +y, -y, +z, -z at `distance` from the origin"""
    eyes = [[distance, 0, 0], [-distance, 0, 0], [0, distance, 0], [0, -distance, 0], [0, 0, distance], [0, 0, -distance]]
    pairs = [rc.look_at(e, [0, 0, 0], H, W, focal) for e in eyes]
    return np.stack([k for k, _ in pairs]), np.stack([r for _, r in pairs])


@functools.lru_cache(maxsize=None)
def general_case(dims=(20, 17, 65), V=8, H=20, W=24, seed=0):
    """A lattice around a sphere of radius 0.6 seen by V ring cameras at distance 3 whose images do not cover the lattice (OUTSIDE) and
    whose near plane, at 2.2, cuts it (BEHIND).  The depth maps are the sphere's with pixels of every kind strewn in: NaN, 0, negative,
    -inf (NODATA), +inf (EMPTY with carve) and a few shifted by more than the band; the weight map has zeros, a NaN, an infinity, a
    negative and otherwise values in (0.25, 1.25)."""
    rng = np.random.default_rng(300 + seed)
    Ks, RTs = tc.ring_cameras(V, H, W, focal=30.0, distance=3.0)
    step = np.array([0.1, 0.1, 0.05])
    lo = -0.5 * step * (np.asarray(dims) - 1) + np.array([-0.05, -0.05, 0.0])
    depth = sphere_depth(Ks, RTs, H, W, 0.6)
    kinds = rng.integers(0, 40, size=depth.shape)
    for k, value in ((0, np.nan), (1, 0.0), (2, -1.5), (3, -np.inf), (4, np.inf)):
        depth[kinds == k] = value
    depth[kinds == 5] -= np.float32(0.75)
    weights = (0.25 + rng.random(depth.shape)).astype(np.float32)
    wk = rng.integers(0, 30, size=depth.shape)
    for k, value in ((0, 0.0), (1, np.nan), (2, np.inf), (3, -1.0), (4, 1e-30)):
        weights[wk == k] = value
    return {"Ks": Ks, "RTs": RTs, "H": H, "W": W, "lo": lo, "step": step, "dims": tuple(dims), "band": 0.25, "z_near": 2.2,
            "depth": depth, "weights": weights}


EXACT_K = np.array([[8.0, 0, 4.0], [0, 8.0, 4.0], [0, 0, 1.0]])
EXACT_RT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def _exact(lo, step, dims, pixel_depth, expect, weights=None, z_near=0.75, carve=True, depth_map=None):
    """one boundary scenario: V identity-pose views of the 9 x 9 exact camera (tc.exact_case: z = p2, x = 8 p0 / p2 + 4 without a
    rounding at z = 1), view v's depth map constant `pixel_depth[v]` (its weight map constant weights[v]); expect: fate [n, V]"""
    V = len(pixel_depth)
    depth = np.empty((V, 9, 9), np.float32)
    depth[:] = np.asarray(pixel_depth, np.float32)[:, None, None]
    if depth_map is not None:
        depth[:] = depth_map
    w = None
    if weights is not None:
        w = np.empty((V, 9, 9), np.float32)
        w[:] = np.asarray(weights, np.float32)[:, None, None]
    return {"Ks": np.stack([EXACT_K] * V), "RTs": np.stack([EXACT_RT] * V), "H": 9, "W": 9, "lo": np.asarray(lo, np.float64),
            "step": np.asarray(step, np.float64), "dims": tuple(dims), "band": 0.25, "z_near": z_near, "carve": carve, "depth": depth,
            "weights": w, "expect": np.asarray(expect, np.int64).reshape(-1, V)}


def boundary_cases():
    """{name: scenario}: every comparison of THE DEFINITION at its edge.  Identity pose and dyadic lattice coordinates: z, s and the
    pixel coordinates are exact, so the expected fate is known without the restatement."""
    one = np.float32(1.0)
    dn = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    point = dict(lo=[0, 0, 1.0], step=[1, 1, 1], dims=(1, 1, 1))              # the point (0, 0, 1): pixel (4, 4), z = 1
    cases = {}
    # s = d - 1 against the band 0.25: -band is NEAR, one ulp below HIDDEN; band is EMPTY, one ulp below NEAR; d of every kind
    cases["depth"] = _exact(**point, pixel_depth=[0.75, dn(0.75), 1.25, dn(1.25), np.nan, np.inf, -np.inf, 0.0],
                            expect=[NEAR, HIDDEN, EMPTY, NEAR, NODATA, EMPTY, NODATA, NODATA])
    cases["depth_no_carve"] = _exact(**point, pixel_depth=[np.inf, -1.0, 3e38, 1.0], carve=False, expect=[NODATA, NODATA, EMPTY, NEAR])
    cases["depth_more"] = _exact(**point, pixel_depth=[-1.0, 3e38, np.float32(1e-45), up(1.25)], expect=[NODATA, EMPTY, HIDDEN, EMPTY])
    # w of every kind at a NEAR pixel (d = 1, s = 0)
    cases["weights"] = _exact(**point, pixel_depth=[1.0] * 6, weights=[0.0, -1.0, np.nan, np.inf, 1e-30, 1.0],
                              expect=[NODATA, NODATA, NODATA, NODATA, NEAR, NEAR])
    cases["weights_tiny_alone"] = _exact(**point, pixel_depth=[1.125], weights=[1e-30], expect=[NEAR])
    # the frame: x = 8 p0 + 4 at z = 1.  p0 = -0.5 and 0.5 are x = 0 and x = 8 = W - 1; one ulp beyond is OUTSIDE
    h = float(up(0.5))
    cases["frame_x"] = _exact(lo=[-0.5, 0, 1.0], step=[1, 1, 1], dims=(2, 1, 1), pixel_depth=[1.0], expect=[NEAR, NEAR])
    cases["frame_y"] = _exact(lo=[0, -0.5, 1.0], step=[1, 1, 1], dims=(1, 2, 1), pixel_depth=[1.0], expect=[NEAR, NEAR])
    cases["frame_corners"] = _exact(lo=[-0.5, -0.5, 1.0], step=[1, 1, 1], dims=(2, 2, 1), pixel_depth=[1.0], expect=[NEAR] * 4)
    cases["beyond_x"] = _exact(lo=[-h, 0, 1.0], step=[2 * h, 1, 1], dims=(2, 1, 1), pixel_depth=[1.0], expect=[OUTSIDE, OUTSIDE])
    cases["beyond_y"] = _exact(lo=[0, -h, 1.0], step=[1, 2 * h, 1], dims=(1, 2, 1), pixel_depth=[1.0], expect=[OUTSIDE, OUTSIDE])
    # the near plane: z = z_near is kept, one ulp under is BEHIND
    cases["near_at"] = _exact(lo=[0, 0, 0.75], step=[1, 1, 1], dims=(1, 1, 1), pixel_depth=[0.75], expect=[NEAR])
    cases["near_under"] = _exact(lo=[0, 0, float(dn(0.75))], step=[1, 1, 1], dims=(1, 1, 1), pixel_depth=[0.75], expect=[BEHIND])
    # pixel coordinates of exactly k + 0.5, k = 0..7, on both axes: rint goes to the even column / row.  The depth map tells which
    # pixel was read: d = 1 + (column - 4) / 64 + (row - 4) / 1024, inside the band, so the value IS that offset
    row, col = np.meshgrid(np.arange(9.0), np.arange(9.0), indexing="ij")
    ramp = (1.0 + (col - 4) / 64 + (row - 4) / 1024).astype(np.float32)
    cases["half_pixels"] = _exact(lo=[-0.4375, -0.4375, 1.0], step=[0.125, 0.125, 1], dims=(8, 8, 1), pixel_depth=[1.0], depth_map=ramp,
                                  expect=[NEAR] * 64)
    even = np.array([0, 2, 2, 4, 4, 6, 6, 8], np.float64)
    cases["half_pixels"]["values"] = ((even[:, None] - 4) / 64 + (even[None, :] - 4) / 1024).astype(np.float32).reshape(8, 8, 1)
    assert one == 1
    return cases


def run_case(case, **kw):
    """restate() on a case dict"""
    args = dict(weights=case.get("weights"), z_near=case.get("z_near", 1e-6), carve=case.get("carve", True))
    args.update(kw)
    return restate(case["depth"], case["Ks"], case["RTs"], case["lo"], case["step"], case["dims"], case["band"], **args)


@functools.lru_cache(maxsize=None)
def sphere_case(H=96, W=96, focal=170.0, distance=6.0, half=1.3, step=0.1, band=0.3, radius=1.0):
    """The analytic unit sphere in six axis cameras whose images cover the lattice [-half, half]^3; "slack_in" and "slack_out": how far
    from the sphere a lattice point must lie for its sign to be decided (derived in tests/test_fusion_host.py)."""
    Ks, RTs = axis_cameras(H, W, focal, distance)
    n = int(round(2 * half / step)) + 1
    z_max = distance + half
    footprint = z_max / focal * np.sqrt(0.5)                     # half a pixel's diagonal at the farthest lattice depth
    d_max = np.sqrt(1.0 + 2.0 * ((max(H, W) - 1) / 2.0 / focal) ** 2)        # the longest pixel direction with camera z 1
    graze = np.sqrt(radius ** 2 + (band * d_max) ** 2) - radius
    return {"Ks": Ks, "RTs": RTs, "H": H, "W": W, "lo": np.full(3, -half), "step": np.full(3, step), "dims": (n, n, n), "band": band,
            "depth": sphere_depth(Ks, RTs, H, W, radius), "radius": radius, "footprint": footprint, "slack_in": footprint,
            "slack_out": graze + footprint}


@functools.lru_cache(maxsize=None)
def convex_case(H=48, W=48, focal=85.0, distance=6.0, half=1.25, step=0.1, band=0.2):
    """icosphere(3) -- convex, vertices on the unit sphere, every face farther than `r_in` from the centre -- in six axis cameras at 48 x
    48 whose images cover the lattice.  margin = the pixel footprint at the farthest lattice depth + one lattice step; cap: the share
    of lattice points within the margin of the unit sphere or of the inner one that a comparison may leave out."""
    v, f = mc.icosphere(3)
    Ks, RTs = axis_cameras(H, W, focal, distance)
    n = int(round(2 * half / step)) + 1
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    nrm = np.cross(b - a, c - a)
    r_in = float(np.abs((nrm * a).sum(axis=1) / np.linalg.norm(nrm, axis=1)).min())
    footprint = (distance + half) / focal * np.sqrt(0.5)
    d_max = np.sqrt(1.0 + 2.0 * ((max(H, W) - 1) / 2.0 / focal) ** 2)
    return {"vertices": v, "faces": f, "Ks": Ks, "RTs": RTs, "H": H, "W": W, "lo": np.full(3, -half), "step": np.full(3, step),
            "dims": (n, n, n), "band": band, "r_in": r_in, "radius": 1.0, "footprint": footprint, "margin": footprint + step,
            "d_max": d_max, "cap": 1.0 / 3.0}


def mesh_depth(case):
    """the CAMERA-Z depth maps of a case's mesh on the host: THE INTERSECTION restated (raycast_cases) along gpnerf_pixel_rays' rays,
    whose directions have camera z 1; +inf where nothing is hit"""
    rays = rc.pixel_rays(case["Ks"], case["RTs"], case["H"], case["W"])
    t = rc.closest_hit(rays.reshape(-1, 8), case["vertices"], case["faces"], np.float32)[0]
    return t.reshape(len(case["Ks"]), case["H"], case["W"]).astype(np.float32)


def squares_case(H=48, W=48, focal=45.0):
    """tc.squares_case's two squares (side 1 at z = 0, side 0.5 at z = 1) seen from z = 3, a lattice of 12 x 10 x 9 dyadic points in the
    front square's shadow between them (z in [0.25, 0.75], more than the band behind the front square and in front of the back one),
    and a side view from x = 3 at their mid height, whose rays through the lattice meet neither square"""
    sq = tc.squares_case()
    K0, RT0 = rc.look_at([0, 0, 3.0], [0, 0, 0], H, W, focal)
    K1, RT1 = rc.look_at([3.0, 0, 0.5], [0, 0, 0.5], H, W, focal)
    return {"vertices": sq["vertices"], "faces": sq["faces"], "Ks": np.stack([K0, K1]), "RTs": np.stack([RT0, RT1]), "H": H, "W": W,
            "lo": np.array([-0.171875, -0.140625, 0.25]), "step": np.array([1 / 32, 1 / 32, 1 / 16]), "dims": (12, 10, 9), "band": 0.125}
