"""GPU: every launch plan of gpnerf_render_fused, run on purpose.

plan_render() (gp-nerf_amd/csrc/gpnerf_kernels.hip) picks one of dozens of launch sequences from the ray count, the sample count,
the flags, the outputs, the device's CU count and the bytes of workspace; tests/test_render_plan.py holds the planner's arithmetic to
its invariants on the host.  Here each reachable plan is rendered: a helper asks frame.render_plan for the plan a candidate call
gets on THIS device (sizes are multiples of its round of wavefronts, not of 256 CUs), every test asserts the plan before it renders
and prints it (-s), and a test that cannot find its plan fails.

Frames are a 64 x 64 synthetic scene's rays repeated modulo the frame, so one oracle render of the 4096 base rays serves every ray of
every case: all rays are compared, which includes the first tile, the last whole tile, the ragged last tile and everything behind
main_rays / in the last partial round.

The DIRECTIONS axis renders the same plans in the flipped sample order (GPNERF_FLAG_FLIP_SAMPLES = raw2outputs(neg=True), what the
dense renderer runs on every THuman frame): `thuman` is the scene with camera space negated, rendered with neg_ray=True (which
flips by default); `flip_only` is the forward scene rendered with flip=True alone, the compositing order without the projector's
sign.  The planner reads neither flag (tests/test_render_plan.py sweeps that), so the forward order's candidate calls get the
forward order's plans; the oracle models every combination and caches one render per (direction, termination)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4          # north_star: max-abs on the maps against the reference CPU path
S = 32
EPS = 1e-5
KEYS = ("rgb_map", "depth_map", "acc_map", "weights", "rgb_in_map")
WANT = ("weights", "z_vals", "rgb_in", "ray_mask")


@pytest.fixture(scope="module")
def fm():
    return importlib.import_module("gp-nerf_amd.frame")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def build_frame(fm, sc):
    return fm.Frame(to_dev(sc["src_imgs"][0]), to_dev(sc["featmaps"]), [to_dev(v) for v in sc["volumes"]], to_dev(sc["src_Ks"][0]),
                    to_dev(sc["src_poses"][0]), sc["Rh"][0], sc["Th"][0], sc["bounds"][0, 0], sc["voxel_size"], sc["out_sh"][0],
                    fm.pack_head(sc["head"], torch.device("cuda:0")))


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ragged(rounds, tiles=0):
    """a ray count: `rounds` rounds of wavefronts of this device + `tiles` 32-ray tiles + a ragged tile of 17 rays"""
    return lambda cus: int(rounds * cus * 8) * 32 + tiles * 32 + 17


SMALL = 48 << 20    # a workspace with room for the tile queue and the chain block, not for a frame's colour list
# Candidate calls per launch shape, cheapest first: (ray count, keyword arguments).  The colour mode and the arithmetic come from
# MODES / FORMS below; the first candidate whose plan on this device is the wanted one is rendered.
SHAPE_CALLS = {
    "STATIC": [(ragged(0.5), {}), (ragged(0.25), {}), (ragged(0, 40), {})],
    # two rounds less a few tiles: more than 1 1/4 rounds, and too large a last round for a remainder launch
    "QUEUE": [(ragged(2, -4), {}), (ragged(1.75), {}), (ragged(2.5), {})],
    # whole rounds + a few tiles: two launches where samples_done is asked for, and from two rounds on
    "QUEUE_REMAINDER": [(ragged(1, 5), {"want": WANT + ("samples_done",)}), (ragged(2, 5), {})],
    "REMAINDER_UNITS": [(ragged(1, 5), {}), (ragged(1, 4), {})],
    # (samples_done: every early-terminated plan is also held to the oracle's run of the same per-ray rule)
    "CHAINED": [(ragged(1, 5), {"early_term": True, "term_eps": EPS, "want": WANT + ("samples_done",)}),
                (ragged(2, -4), {"early_term": True, "term_eps": EPS, "want": WANT + ("samples_done",)})],
}
MODES = {
    "STEP": [{"exits": False}],
    "WAVE": [{"workspace_cap": SMALL}, {"workspace_cap": 1 << 20}, {"workspace_cap": 4 << 20}, {}],
    "LIST": [{"shared_device": True}, {}],
    "UNIFIED": [{}],
}
FORMS = {"REF": {}, "FOLD": {"fold": True}, "SPLIT": {"split_f16": True, "guard": False}, "GUARD": {"split_f16": True, "guard": True}}
# tests/test_render_plan.py REACHABLE, reference-order form: 16 (shape, colour) pairs
REF_PAIRS = [(sh, co) for sh in SHAPE_CALLS for co in MODES if co in ("STEP", "WAVE") or (co == "LIST" and sh != "STATIC") or
             (co == "UNIFIED" and sh in ("QUEUE", "REMAINDER_UNITS"))]


def find_plan(fm, shape, colour, sel, extra=None, modes=None):
    """(n_rays, kwargs, plan) of the first candidate call whose plan on this device is (shape, colour, sel); colour may be a tuple:
    any of them.  modes: the keyword arguments to try instead of MODES[colour].  Fails, with what every candidate got instead, when
    there is none."""
    colours = (colour,) if isinstance(colour, str) else colour
    extra = dict(extra or {})
    tried = []
    for n_of, kw_shape in SHAPE_CALLS[shape]:
        for kw_mode in (modes if modes is not None else [m for co in colours for m in MODES[co]]):
            kw = dict(kw_shape, **kw_mode, **FORMS[sel])
            kw.update({k: v for k, v in extra.items() if k != "want"})
            want = tuple(dict.fromkeys(kw_shape.get("want", WANT) + extra.get("want", ())))
            kw["want"] = tuple(w for w in want if not w.startswith("-") and "-" + w not in want)      # ("-weights": without them)
            n = n_of(n_cus())
            plan = fm.render_plan(None, n, S, **kw)
            t = plan.triple()
            if t[0] == shape and t[1] in colours and t[2] == sel:
                print(f"\n  plan: n_rays={n} S={S} {kw} -> {plan}")
                return n, kw, plan
            tried.append((n, kw, t))
    pytest.fail(f"no candidate call gets the plan {(shape, colour, sel)} on {n_cus()} CUs: {tried}")


# direction -> (render_fused's keywords, oracle.render's keywords)
DIRECTIONS = {
    "forward": ({}, {}),
    "thuman": ({"neg_ray": True}, {"neg_ray": True}),                       # flip defaults to neg_ray on both sides
    "flip_only": ({"flip": True, "neg_ray": False}, {"flip": True}),
}
SCENE_KW = dict(H=64, W=64, seed=9, fill="full", pose="identity", sigma_bias=1.0)


class Scene:
    """a 64 x 64 scene on the device, its base rays, the render keywords of its direction, and the oracle's render of the rays in
    that direction (cached per termination setting).  like: a Scene of the same data, whose frame and rays this one shares."""

    def __init__(self, fm, oracle, sc, direction="forward", like=None, stages=False, **oracle_kw):
        self.fm, self.oracle, self.sc, self.direction, self.stages = fm, oracle, sc, direction, stages
        self.kw, self.okw = (dict(d) for d in DIRECTIONS[direction])
        self.okw.update(oracle_kw)
        self.fr = like.fr if like is not None else build_frame(fm, sc)
        self.rays_h = oracle.rays_of(sc)
        self.base = like.base if like is not None else to_dev(self.rays_h)
        self._ref = {}

    def rays(self, n):
        return self.base[torch.arange(n, device=self.base.device) % self.base.shape[0]].contiguous()

    def ref(self, term_eps=0.0):
        if term_eps not in self._ref:
            ref = self.oracle.render(self.sc, S, term_eps=term_eps, stages=self.stages and not term_eps, **self.okw)
            for k in ("st_grid", "st_vol_feat", "st_rgb_feat", "st_mask"):      # (of the stages only st_raw is compared)
                ref.pop(k, None)
            if term_eps:
                # the scene terminates: nearly every ray stops early, well before the middle of the ray on average.  (The rule is
                # the kernel's per-ray one, flip included: a ray stops at the first step at whose start its T is below term_eps.)
                done = ref["samples_done"]
                early, mean = float((done < S).mean()), float(done.mean()) / S
                print(f"\n  oracle, {self.direction}, term_eps={term_eps}: {early:.4f} of the rays stop early, after {mean:.3f} S samples on average")
                assert early > 0.9 and mean < 0.6, (self.direction, early, mean)
            self._ref[term_eps] = ref
        return self._ref[term_eps]


def moved(a, b):
    """per ray: the largest change of any of its components"""
    d = np.abs(a - b)
    return d.reshape(d.shape[0], -1).max(1)


@pytest.fixture(scope="module")
def scene(fm, syn, oracle):
    sc = syn.make_scene(**SCENE_KW)
    s = Scene(fm, oracle, sc)
    assert float(s.rays_h[:, 7].max()) * EPS < 5e-5      # early termination drops at most term_eps * far of the depth
    return s


def flipping_matters(fwd, flp, tag):
    """the flipped oracle render of a scene against its forward one: a kernel that ignored the flag, or applied it to the wrong
    operand, is far outside TOL on (nearly) every ray"""
    rgb, rin, w = moved(fwd["rgb_map"], flp["rgb_map"]), moved(fwd["rgb_in_map"], flp["rgb_in_map"]), moved(fwd["weights"], flp["weights"])
    nz = float((flp["weights"] != 0).mean())
    print(f"\n  {tag}: flipping moves rgb_map by {rgb.min():.3g}..{rgb.max():.3g}, rgb_in_map by > 1e-2 on {(rin > 1e-2).mean():.3f} of the rays, "
          f"weights by up to {w.max():.3g}; {nz:.3f} of the flipped weights are non-zero")
    assert rgb.min() > 1e-2 and (rin > 1e-2).mean() > 0.95 and w.max() > 0.5 and nz > 0.8, tag


@pytest.fixture(scope="module")
def thuman(fm, syn, oracle, scene):
    """The scene with camera space negated (THuman's convention), rendered as build_render renders THuman: neg_ray, which flips.
    Preconditions, on the oracle's own outputs and before any GPU call: negating the cameras changes nothing else (un-flipped, the
    render is the forward one bit for bit), flipping changes every ray, and without neg_ray no view sees the scene."""
    sc = syn.make_scene(neg_cams=True, **SCENE_KW)
    s = Scene(fm, oracle, sc, "thuman", stages=True)
    assert np.array_equal(s.rays_h, scene.rays_h)
    fwd, flp = scene.ref(), s.ref()
    unflipped = oracle.render(sc, S, neg_ray=True, flip=False)
    for k in unflipped:
        assert np.array_equal(unflipped[k].view(np.uint8), fwd[k].view(np.uint8)), ("neg_cams changes more than the sign of camera space", k)
    flipping_matters(fwd, flp, "thuman")
    assert float(oracle.render(sc, S, neg_ray=False)["acc_map"].max()) == 0.0
    assert float(s.rays_h[:, 7].max()) * EPS < 5e-5
    return s


@pytest.fixture(scope="module")
def flip_only(fm, oracle, scene):
    """The forward scene and frame, composited in the flipped order: flip=True, neg_ray=False."""
    s = Scene(fm, oracle, scene.sc, "flip_only", like=scene)
    flipping_matters(scene.ref(), s.ref(), "flip_only")
    return s


@pytest.fixture
def in_direction(request, scene):
    """direction name -> its Scene (the flipped ones are built, and their oracle renders made, only where a case asks)"""
    return lambda d: scene if d == "forward" else request.getfixturevalue(d)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def against_the_oracle(scene, n, kw, plan):
    """render the call in the scene's direction; every ray against the oracle's render of its base ray in that direction
    (early-terminated plans against the UNTERMINATED oracle: rgb / acc lose at most T_stop <= term_eps, depth at most
    term_eps * far -- tests/test_gpu_configs.py config 3 -- and against the oracle terminated by the same rule, below)"""
    fm = scene.fm
    rays = scene.rays(n)
    assert all(kw.get(k) == v for k, v in scene.kw.items()), (scene.direction, kw)
    got = fm.render_fused(scene.fr, rays, S, **kw)
    ref = scene.ref()
    rows = np.arange(n) % scene.rays_h.shape[0]
    host = {k: v.cpu().numpy() for k, v in got.items()}
    for k in KEYS:
        err = float(np.abs(host[k] - ref[k][rows]).max())
        print(f"    {scene.direction} {k}: max error against the oracle {err:.3g}")
        assert err < TOL, (k, err, str(plan))
    # what must NOT flip (z_vals: raw2outputs flips rgb and sigma, not z) and what counts the samples in whatever order
    err = float(np.abs(host["z_vals"] - ref["z_vals"][rows]).max())
    print(f"    {scene.direction} z_vals: max error against the oracle {err:.3g}")
    assert err <= 1e-6, ("z_vals", err, str(plan))
    if kw.get("early_term"):
        # ... and against the oracle run with the SAME per-ray rule (oracle.render(term_eps=)): the maps and the weights to 2e-5, the
        # figure tests/test_gpu_configs.py config 3 holds this comparison to; the same stopping sample on at least 98 % of the rays
        # (a cap, not a tolerance: a ray whose T sits within float32 rounding of term_eps at a sample boundary may stop one sample
        # apart -- two float32-equivalent evaluations of the oracle's own rule disagree on 4 of these 4096 rays), and where the
        # stopping sample is the same, the same ray_mask (which counts the samples a ray evaluated)
        assert kw["term_eps"] == EPS and "samples_done" in got, kw
        ref_t = scene.ref(EPS)
        for k in KEYS:
            err = float(np.abs(host[k] - ref_t[k][rows]).max())
            print(f"    {scene.direction} {k}: max error against the oracle's per-ray termination {err:.3g}")
            assert err < 2e-5, (k, err, str(plan))
        same = host["samples_done"] == ref_t["samples_done"][rows]
        print(f"    {scene.direction} samples_done: differs from the oracle's on {1 - same.mean():.5f} of the rays")
        assert same.mean() >= 0.98, (float(same.mean()), str(plan))
        assert np.array_equal(host["ray_mask"][same].astype(bool), ref_t["ray_mask"][rows][same].astype(bool)), str(plan)
        assert float((host["samples_done"] < S).mean()) > 0.9 and float(host["samples_done"].mean()) < 0.6 * S
    else:
        assert np.array_equal(host["ray_mask"].astype(bool), ref["ray_mask"][rows].astype(bool)), str(plan)
    if "raw" in host:        # the store index (sample ks, not composite step k): the oracle's per-sample head outputs, un-flipped
        err = float(np.abs(host["raw"] - ref["st_raw"][rows]).max())
        print(f"    {scene.direction} raw: max error against the oracle {err:.3g}")
        assert err < TOL, ("raw", err, str(plan))
    # the tail the remainder shapes exist for: at least 128 rays behind main_rays / in the last partial round, and something is
    # rendered there at all
    slots = plan.n_cus * 8
    if plan.triple()[0] == "QUEUE_REMAINDER":
        assert 128 <= n - plan.main_rays, str(plan)
    if plan.triple()[0] == "REMAINDER_UNITS":
        assert 128 <= n - plan.tiles // slots * slots * 32 <= slots * 4, str(plan)
    tail = plan.main_rays if plan.main_rays < n else n - 128
    assert float(got["acc_map"][tail:].max()) > 0.1
    # One wavefront per whole tile, fp32: the bits do not depend on the launch (include/gpnerf_hip.h `workspace`).  Not the chained
    # launches, which stop a ray where a launch without a workspace stops its 32-ray tile.
    if plan.split == 1 and plan.triple()[2] in ("REF", "FOLD") and not kw.get("early_term"):
        whole = fm.render_fused(scene.fr, rays, S, load_balance=False, **{k: v for k, v in kw.items() if k != "workspace_cap"})
        for k in got:
            assert torch.equal(bits(got[k]), bits(whole[k])), (k, str(plan))
    return got


def direction_cases(cases, directions=("forward", "thuman")):
    """(case..., direction) for pytest.mark.parametrize: the forward cases keep the ids they had before the axis existed"""
    params = []
    for d in directions:
        for c in cases:
            c = c if isinstance(c, tuple) else (c,)
            params.append(pytest.param(*c, d, id="-".join(c) + ("" if d == "forward" else "-" + d)))
    return params


@pytest.mark.parametrize("shape,colour,direction", direction_cases(REF_PAIRS))
def test_every_reachable_plan_of_the_reference_order_form_against_the_oracle(shape, colour, direction, fm, in_direction):
    scene = in_direction(direction)
    n, kw, plan = find_plan(fm, shape, colour, "REF", extra=scene.kw)
    assert plan.triple() == (shape, colour, "REF")
    if shape == "STATIC":
        assert plan.split > 1, "the static candidates are frames that split a tile's samples"
    against_the_oracle(scene, n, kw, plan)


@pytest.mark.parametrize("shape,sel,direction", direction_cases([(sh, sel) for sel in ("FOLD", "SPLIT") for sh in SHAPE_CALLS]))
def test_the_folded_and_the_split_form_on_every_launch_shape_against_the_oracle(shape, sel, direction, fm, in_direction):
    scene = in_direction(direction)
    n, kw, plan = find_plan(fm, shape, ("UNIFIED", "LIST", "WAVE"), sel, extra=scene.kw, modes=[{}])
    assert plan.triple()[0] == shape and plan.triple()[2] == sel
    against_the_oracle(scene, n, kw, plan)


# the most deferred colour form each launch shape reaches (tests/test_render_plan.py REACHABLE)
MOST_DEFERRED = {"STATIC": "WAVE", "QUEUE": "UNIFIED", "QUEUE_REMAINDER": "LIST", "REMAINDER_UNITS": "UNIFIED", "CHAINED": "LIST"}


@pytest.mark.parametrize("shape", list(SHAPE_CALLS))
def test_the_flipped_sample_order_alone_on_every_launch_shape_against_the_oracle(shape, fm, flip_only):
    """GPNERF_FLAG_FLIP_SAMPLES without GPNERF_FLAG_NEG_RAY, on the forward scene: the compositing order apart from the projector's
    sign.  The ABI takes the two flags separately; only render_fused's default ties them."""
    n, kw, plan = find_plan(fm, shape, MOST_DEFERRED[shape], "REF", extra=flip_only.kw)
    assert plan.triple() == (shape, MOST_DEFERRED[shape], "REF") and kw["flip"] is True and kw["neg_ray"] is False
    against_the_oracle(flip_only, n, kw, plan)


def test_raw_is_stored_at_the_sample_index_under_the_flipped_order(fm, thuman):
    """A `raw` output keeps the colour branch in the step (Colour::STEP) and is written at the SAMPLE's index: composite step k
    evaluates sample S-1-k and stores it there.  The oracle's st_raw is per sample, un-flipped; its first and last samples differ
    on every ray, so a store at the composite step's index cannot pass."""
    st = thuman.ref()["st_raw"]
    ends, rev = moved(st[:, 0], st[:, S - 1]), moved(st, st[:, ::-1])
    print(f"\n  oracle st_raw: first and last sample differ by {ends.min():.3g}..{ends.max():.3g}; reversed along the ray it moves by >= {rev.min():.3g}")
    assert ends.min() > 1e-2 and rev.min() > 1e-2
    n, kw, plan = find_plan(fm, "QUEUE", "STEP", "REF", extra=dict(thuman.kw, want=("raw",)), modes=[{}])
    assert plan.triple() == ("QUEUE", "STEP", "REF") and "raw" in kw["want"]
    got = against_the_oracle(thuman, n, kw, plan)
    assert "raw" in got


def overflow_scene(syn, **scene_kw):
    """tests/test_gpu_guard.py's overflow data, both kinds at once: huge source-view features in the left third of the views and a
    huge volume level in a corner -- MFMA operands of the split form leave the f16 range in part of the image.  Wrong VALUES in the
    unguarded split form (inf / NaN in registers), never an address."""
    sc = dict(syn.make_scene(H=64, W=64, seed=5, fill="full", pose="identity", **scene_kw))
    f = sc["featmaps"].copy()
    f[:, :, : f.shape[2] // 3] *= 3.0e5
    sc["featmaps"] = f
    v = [a.copy() for a in sc["volumes"]]
    v[1][..., : v[1].shape[-2] // 3, : v[1].shape[-1] // 3] *= 2.0e5
    sc["volumes"] = v
    return sc


@pytest.fixture(scope="module")
def overflow(fm, syn, oracle):
    return Scene(fm, oracle, overflow_scene(syn))


@pytest.fixture(scope="module")
def overflow_thuman(fm, syn, oracle):
    """the overflow data seen by negated cameras: rendered with neg_ray, the guard's fix-up launch runs flipped on flagged tiles"""
    return Scene(fm, oracle, overflow_scene(syn, neg_cams=True), "thuman")


GUARD_CASES = [("STATIC", {}), ("QUEUE", {}), ("QUEUE_REMAINDER", {}), ("REMAINDER_UNITS", {}), ("CHAINED", {}),
               ("QUEUE", {"ray_order": True}), ("QUEUE", {"occ_cull": True}), ("QUEUE_REMAINDER", {"thuman": True}), ("CHAINED", {"thuman": True})]


@pytest.mark.parametrize("shape,how", GUARD_CASES, ids=[s + "".join("-" + k for k in h) for s, h in GUARD_CASES])
def test_the_guard_with_tiles_flagged_on_every_launch_shape(shape, how, fm, overflow, request):
    """GPNERF_FLAG_SPLIT_GUARD's one promise -- the result never depends on the range of the data -- on every launch shape, with
    flagged tiles in the first round, the last whole round and the remainder (the scene's rays repeat every 4096), in a random ray
    order, and under the occupancy cull's mask and tile order (the fix-up launch has an instantiation of its own for it).

    The fix-up launch has to walk every tile of the call whatever the render launches' cut into rounds and a remainder: under
    QUEUE_REMAINDER the second launch flags its tiles by their slot in the whole call, behind main_rays.

    thuman: the same data seen by negated cameras and rendered with neg_ray, flipped: FORM_F32_FIXUP in the flipped order, behind
    main_rays and on the chained launches' tiles (the fp32 form it is held to is the oracle's in test_every_reachable_plan...)."""
    extra = {"want": ("guard_tiles",)}
    if how.get("thuman"):
        overflow = request.getfixturevalue("overflow_thuman")
        extra.update(overflow.kw)
    if how.get("occ_cull"):
        extra.update(occ_cull=True, want=("guard_tiles", "-weights"))
    n, kw, plan = find_plan(fm, shape, "WAVE", "GUARD", extra=extra, modes=[{}])
    assert plan.triple() == (shape, "WAVE", "GUARD") and plan.regions().get("guard"), str(plan)
    assert (plan.split > 1) == (shape == "STATIC") and bool(plan.regions().get("mask")) == bool(how.get("occ_cull")), str(plan)
    kw = {k: v for k, v in kw.items() if k not in ("split_f16", "guard")}
    rays = overflow.rays(n)
    if how.get("ray_order"):
        kw["ray_order"] = torch.randperm(n, generator=torch.Generator().manual_seed(3)).int().cuda()
    fr = overflow.fr
    ref = fm.render_fused(fr, rays, S, fold=False, **kw)                               # the fp32 form as the fix-up launch runs it
    bad = fm.render_fused(fr, rays, S, split_f16=True, guard=False, **kw)
    got = fm.render_fused(fr, rays, S, split_f16=True, guard=True, **kw)
    flagged = int(got["guard_tiles"])
    if how.get("thuman"):       # the flipped order with real density: un-flipped, the same call gives another image
        assert kw["neg_ray"] is True and "flip" not in kw
        unflipped = fm.render_fused(fr, rays, S, fold=False, flip=False, **kw)
        d = (unflipped["rgb_map"] - ref["rgb_map"]).abs().nan_to_num(nan=0.0).max(1).values
        print(f"    flipping moves rgb_map by > 1e-2 on {float((d > 1e-2).float().mean()):.3f} of the rays; acc_map up to {float(ref['acc_map'].max()):.3g}")
        assert float((d > 1e-2).float().mean()) > 0.5 and float(ref["acc_map"].max()) > 0.1
    # the last partial round (QUEUE_REMAINDER: what the second launch renders)
    slots = plan.n_cus * 8
    tail = int(plan.main_rays) if shape == "QUEUE_REMAINDER" else (plan.tiles - 1) // slots * slots * 32
    assert n - tail >= 128
    keys = [k for k in KEYS if k in got]
    err_bad = {where: float((bad["rgb_map"][sl] - ref["rgb_map"][sl]).abs().nan_to_num(nan=1e9).max())
               for where, sl in (("first tiles", slice(0, 4096)), ("tail", slice(tail, n)))}
    err = {k: float((got[k] - ref[k]).abs().nan_to_num(nan=1e9).max()) for k in keys}
    err_tail = {k: float((got[k][tail:] - ref[k][tail:]).abs().nan_to_num(nan=1e9).max()) for k in keys}
    print(f"    guard_tiles={flagged} of {plan.tiles}; unguarded split form off by {err_bad}; guarded: max error {err}; behind ray {tail}: {err_tail}")
    assert 0 < flagged <= plan.tiles, (flagged, plan.tiles)
    assert int(ref["guard_tiles"]) == 0 and int(bad["guard_tiles"]) == 0
    # without the guard the split form is simply wrong on this data, in the first round and in the tail
    assert err_bad["first tiles"] > 1e-2 and err_bad["tail"] > 1e-2, err_bad
    for k in keys:
        assert err[k] < TOL, (k, err[k], "behind main_rays / in the last partial round:", err_tail[k], "guard_tiles", flagged, str(plan))
    assert torch.equal(got["z_vals"], ref["z_vals"])
    if kw.get("early_term"):
        return      # the fix-up launch terminates per tile, the chained launch per ray: equal to the bound above, not to the bit
    # the flagged tiles ARE the fp32 form's, bit for bit: the fix-up launch runs the same code on the same 32 rays of a launch slot
    whole = fm.render_fused(fr, rays, S, load_balance=False, fold=False, **{k: v for k, v in kw.items() if k != "want"})
    diff = (got["rgb_map"] != whole["rgb_map"]).any(1)
    if "ray_order" in kw:
        diff = diff[kw["ray_order"].long()]
    pad = torch.zeros(plan.tiles * 32, dtype=torch.bool, device=diff.device)
    pad[: diff.numel()] = diff
    assert int((~pad.view(plan.tiles, 32).any(1)).sum()) >= flagged


def test_the_keep_bit_mask_in_the_flipped_order_on_the_tile_queue(fm, syn, oracle):
    """GPNERF_FLAG_OCC_CULL | GPNERF_FLAG_FLIP_SAMPLES on the tile queue with the keep bits in the workspace (Loop::CULLED):
    occupancy_mask_kernel has to put composite step k's bit at the occupancy of sample S-1-k.  No caller of the project's renders
    this (the progressive renderer never flips), the ABI takes it and the oracle models it: oracle.render(occ=, flip=True).
    On the oracle's outputs first: culling removes a good part of the samples that have density, not all, and the flipped culled
    weights are far from the un-flipped ones on most rays that have any."""
    sc = syn.make_scene(vol_occupancy=0.35, **SCENE_KW)
    occ = oracle.build_occupancy(sc)
    dense = oracle.render(sc, S, stages=True)["st_raw"][..., 3] > 0
    fwd = oracle.render(sc, S, occ=occ, stages=True)
    removed = float((dense & (fwd["st_raw"][..., 3] == 0)).sum() / dense.sum())
    s = Scene(fm, oracle, sc, "flip_only", occ=occ)
    ref = s.ref()
    has = (fwd["weights"].sum(1) > 0) | (ref["weights"].sum(1) > 0)
    far = float((moved(fwd["weights"], ref["weights"])[has] > 1e-2).mean())
    print(f"\n  oracle: culling removes {removed:.3f} of the samples with density; {has.mean():.3f} of the rays keep weight, flipping moves {far:.3f} of those by > 1e-2")
    assert 0.2 < removed < 0.8 and has.mean() > 0.5 and far >= 0.5
    n, kw, plan = find_plan(fm, "QUEUE", "WAVE", "REF", extra=dict(s.kw, occ_cull=True, want=("-weights",)), modes=[{}])
    assert plan.triple() == ("QUEUE", "WAVE", "REF") and plan.regions().get("mask") and "weights" not in kw["want"], str(plan)
    occ_dev = s.fr.build_occupancy().cpu().numpy()
    assert float(np.abs(occ_dev - occ).max()) < 1e-4
    got = fm.render_fused(s.fr, s.rays(n), S, **kw)
    rows = np.arange(n) % s.rays_h.shape[0]
    for k in ("rgb_map", "depth_map", "acc_map", "rgb_in_map"):
        err = float(np.abs(got[k].cpu().numpy() - ref[k][rows]).max())
        print(f"    culled, flipped {k}: max error against the oracle {err:.3g}")
        assert err < TOL, (k, err, str(plan))
    assert float(np.abs(got["z_vals"].cpu().numpy() - ref["z_vals"][rows]).max()) <= 1e-6
    assert np.array_equal(got["ray_mask"].cpu().numpy().astype(bool), ref["ray_mask"][rows].astype(bool))
    # the in-loop test of the same call (a `weights` output keeps the mask out of the launch): the same bits, and the weights
    loop = fm.render_fused(s.fr, s.rays(n), S, **dict(kw, want=kw["want"] + ("weights",)))
    assert not fm.render_plan(None, n, S, **dict(kw, want=kw["want"] + ("weights",))).regions().get("mask")
    for k in got:
        assert torch.equal(bits(got[k]), bits(loop[k])), k
    err = float(np.abs(loop["weights"].cpu().numpy() - ref["weights"][rows]).max())
    print(f"    culled, flipped weights (in-loop test): max error against the oracle {err:.3g}")
    assert err < TOL


def test_a_captured_guarded_call_clears_the_previous_replays_flags(fm, overflow):
    """The guarded split form on overflow data, a frame with a remainder launch, captured into a HIP graph: three replays give the
    same bits and the same positive guard_tiles.  Before every replay the test sets every tile's flag word in the guard region (at
    the offset render_plan reports, in the module's cached workspace of the capture stream): a replay that did not clear them would
    count every tile."""
    n, kw, plan = find_plan(fm, "QUEUE_REMAINDER", "WAVE", "GUARD", extra={"want": ("guard_tiles",)}, modes=[{}])
    assert plan.triple() == ("QUEUE_REMAINDER", "WAVE", "GUARD") and plan.main_rays < n, str(plan)
    g_off, g_bytes = plan.regions()["guard"]
    rays = overflow.rays(n)
    ref = fm.render_fused(overflow.fr, rays, S, **kw)
    flagged = int(ref["guard_tiles"])
    assert 0 < flagged < plan.tiles
    fp32 = fm.render_fused(overflow.fr, rays, S, fold=False, **{k: v for k, v in kw.items() if k not in ("split_f16", "guard")})
    for k in KEYS:              # (the replays below are held to ref's bits: ref itself is the fp32 form's to the usual bound, remainder included)
        assert float((ref[k] - fp32[k]).abs().nan_to_num(nan=1e9).max()) < TOL, k
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fm.render_fused(overflow.fr, rays, S, **kw)              # warm-up on the capture stream (allocator pool, kernel attributes)
        ws = fm._workspace(rays.device, 0)                       # the capture stream's cached workspace
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = fm.render_fused(overflow.fr, rays, S, **kw)
    with torch.cuda.stream(s):
        assert fm._workspace(rays.device, 0).data_ptr() == ws.data_ptr() and ws.numel() >= g_off + g_bytes
    words = ws[g_off:g_off + g_bytes].view(torch.int32)
    assert 64 + plan.tiles <= words.numel()
    for i in range(3):
        for v in out.values():
            v.zero_()
        words[64:64 + plan.tiles] = 1                           # (word 0: the count; words 64..: one flag per tile)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(out["guard_tiles"]) == flagged, (i, int(out["guard_tiles"]), flagged)
        for k in ref:
            assert torch.equal(bits(out[k]), bits(ref[k])), (i, k)
